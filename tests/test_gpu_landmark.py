"""GPU: shortest paths from device triples and the landmark start built on them (docs/SPEC.md
2.1.2, 2.5.4; `bb_triples_paths`, `bb_paths_*`, `landmark_start`, `StructureSolver(init=
'landmark')`).

The reference is tests/_landmark_model.py -- edge weights by the rules of tests/_input_model.py,
geodesics by scipy.sparse.csgraph.dijkstra, the landmark rule and the placement sum in numpy --
never the library.  The distances are held to scipy's BITS: the fixed point of d[v] = min(d[v],
fl(d[u] + w)) is unique (tests/test_landmark_cpu.py), so no order of relaxation can change it.
Counts are 4^-k, k = 0 .. 5, under alpha = 1: the device's pow() returns their reciprocals
exactly, so that the WEIGHTS are the model's bits too.  It does not for every power of two (probed
on the MI355X: one ulp low at 2^-11, 2^4, 2^9, 2^12, ...), so counts divided by KR vectors are held
to SPEC 4's pow tolerance against the model and bit for bit to the device's own result on the list
divided beforehand.  'wish' maps carry arbitrary doubles and arbitrary KR vectors (a division is
the same everywhere).  A +inf cell is the largest double after nan_to_num, as for every triple route
(an edge like any other); NaN, 0, -inf and negative cells are no edge.

Sizes.  A wave takes one segment of 1,024 entries of a row and one chunk of 64 sources: node
counts around 64, source counts around the chunk (1, 3, 64, 65, 130), a row of 1,500 entries
(two segments), a path graph of 299 edges in a row (more sweeps than one batch of 8 holds unless
the waves happen to run in path order)."""
import numpy
import pytest

import blueberry_amd as bb
from blueberry_amd import _lib
from tests import _input_model as im
from tests import _landmark_model as lm
from tests._util import bits

pytestmark = pytest.mark.gpu

SOURCE_COUNTS = (1, 3, 64, 65, 130)


def sources_for(n_nodes, count, seed):
    """`count` sources in random order; with repeats once there are more of them than nodes."""
    return numpy.random.default_rng(seed).integers(0, n_nodes, count)


COUNTS_POW_TOL = 1e-12      # SPEC 4: device pow() against numpy's, float64


def check_paths(triples, resolution, n_nodes, sources, kind="wish", alpha=3.0, kr=None, ke=None,
                dev=None, w=None, pow_tol=None):
    """shortest_paths and edge_degrees of one input against the model, bit for bit; returns the
    device's rows on the host.  pow_tol: the weights went through the device's pow() on values
    where it need not be exact -- the lengths then agree within n 2^-52 + pow_tol relative (sums
    of at most n - 1 positive terms, min exact: tests/test_gpu_shortest_paths.py) and everything
    else exactly."""
    if w is None:
        w = lm.weights_of(triples, resolution, n_nodes, kind=kind, alpha=alpha, kr=kr, ke=ke)
    g = lm.geodesics(w, sources)
    own = dev is None
    if own:
        dev = bb.DeviceTriples(triples, resolution, 0)
    try:
        deg = dev.edge_degrees(n_nodes, kind=kind, alpha=alpha, KRnorm=kr, KRexpected=ke)
        assert deg.dtype == numpy.int64 and numpy.array_equal(deg, lm.edge_degrees_of(w))
        with dev.shortest_paths(n_nodes, sources, kind=kind, alpha=alpha, KRnorm=kr, KRexpected=ke) as rows:
            got = rows.to_host()
            assert got.shape == (len(sources), n_nodes)
            if pow_tol is None:
                assert numpy.array_equal(bits(got), bits(lm.as_read(g)))
            else:
                want = lm.as_read(g)
                rel = numpy.abs(got - want) / numpy.maximum(want, 1e-300)
                print("%s with pow(): worst relative difference %.3e (bound %.3e)"
                      % (kind, rel.max(), n_nodes * 2.0 ** -52 + pow_tol))
                assert ((got == 0) == (want == 0)).all()
                assert rel.max() <= n_nodes * 2.0 ** -52 + pow_tol
                g = numpy.where(got == 0, g, got)                # (for the reads below)
            assert rows.unreachable_ == int(numpy.isinf(g).sum())
            assert 0 <= rows.sweeps_ <= n_nodes and (rows.sweeps_ >= 1 or not (w > 0).any())
            assert numpy.array_equal(rows.reached(), (~numpy.isinf(g)).sum(axis=1))
            pick = numpy.random.default_rng(5).integers(0, n_nodes, 7)
            assert numpy.array_equal(bits(rows.columns(pick)), bits(lm.as_read(g)[:, pick]))
            assert rows.columns([]).shape == (len(sources), 0)
    finally:
        if own:
            dev.close()
    return got


# ---- 1. bits, at every edge of the node and source counts --------------------------------------
@pytest.mark.parametrize("n_nodes", [1, 2, 63, 64, 65, 300, 1600])
def test_random_graphs_bit_for_bit(n_nodes):
    m = max(1, 3 * n_nodes)
    triples = lm.random_graph_triples(n_nodes, m, seed=n_nodes)
    if n_nodes == 2:
        triples[0, :2] = (0.0, 1.0)                     # at least one edge
    w = lm.weights_of(triples, 1, n_nodes, kind="wish")
    dev = bb.DeviceTriples(triples, 1, 0)
    for count in SOURCE_COUNTS:
        check_paths(triples, 1, n_nodes, sources_for(n_nodes, count, count), dev=dev, w=w)
    dev.close()


def test_an_empty_list_and_a_graph_without_edges():
    for triples in (numpy.zeros((0, 3)), numpy.array([[2.0, 2.0, 1.0], [0.0, 1.0, 0.0]])):
        got = check_paths(triples, 1, 5, [3, 0, 3])
        assert not got.any()


@pytest.mark.parametrize("kind", ["wish", "counts"])
@pytest.mark.parametrize("with_kr", [False, True])
@pytest.mark.parametrize("order", ["C", "F"])
def test_kinds_kr_vectors_and_both_memory_orders(kind, with_kr, order):
    n_nodes, res = 300, 5000
    rng = numpy.random.default_rng(17)
    alpha = 3.0 if kind == "wish" else 1.0
    t = lm.random_graph_triples(n_nodes, 1200, seed=3, resolution=res, wish=kind == "wish")
    t[:, :2] += rng.integers(0, res, t[:, :2].shape)                 # anywhere inside the bin
    kr = ke = None
    if with_kr:
        if kind == "wish":
            kr, ke = rng.uniform(0.5, 2.0, n_nodes - 1), rng.uniform(0.5, 2.0, n_nodes - 1)
            kr[rng.random(n_nodes - 1) < 0.03] = numpy.nan           # (bin n_nodes - 1: padded NaN)
        else:
            kr, ke = im.pow2_kr(n_nodes - 1, seed=1)
    triples = numpy.asfortranarray(t) if order == "F" else numpy.ascontiguousarray(t)
    sources = sources_for(n_nodes, 70, 2)
    if not (with_kr and kind == "counts"):
        check_paths(triples, res, n_nodes, sources, kind=kind, alpha=alpha, kr=kr, ke=ke)
        return
    # counts / KR leaves powers of two whose reciprocal the device's pow() does not always hit
    # exactly (see the top of the file): the model within the pow tolerance, and bit for bit the device's own
    # result for the list divided beforehand, without KR vectors
    got = check_paths(triples, res, n_nodes, sources, kind=kind, alpha=alpha, kr=kr, ke=ke,
                      pow_tol=COUNTS_POW_TOL)
    rows, cols = im.bins_of(t[:, 0], res), im.bins_of(t[:, 1], res)
    lo, hi = numpy.minimum(rows, cols), numpy.maximum(rows, cols)
    divided = t.copy()
    divided[:, 2] = im._kr_quotient(t[:, 2], lo, hi, im._pad(kr, n_nodes), im._pad(ke, n_nodes))
    with bb.DeviceTriples(divided, res, 0).shortest_paths(n_nodes, sources, kind=kind, alpha=alpha) as plain:
        assert numpy.array_equal(bits(plain.to_host()), bits(got))


def test_a_path_graph_needs_many_sweeps():
    """Nearest neighbours only: 299 edges in a row.  Relaxing in place, the number of sweeps
    depends on the order the waves run in -- anywhere from 2 to 300 -- and is only bounded."""
    n = 300
    rng = numpy.random.default_rng(8)
    i = numpy.arange(n - 1, dtype=numpy.float64)
    triples = numpy.stack([i, i + 1, rng.uniform(0.5, 1.5, n - 1)], axis=1)
    for sources in ([0], [n - 1, 0, 150], sources_for(n, 65, 1)):
        check_paths(triples, 1, n, sources)


def test_a_hub_row_spans_two_segments():
    n = 1600
    rng = numpy.random.default_rng(4)
    spokes = rng.permutation(numpy.arange(1, n))[:1500].astype(numpy.float64)
    hub = numpy.stack([numpy.full(1500, 0.0), spokes, rng.uniform(1.0, 3.0, 1500)], axis=1)
    hub[::2, :2] = hub[::2, 1::-1]                                   # either orientation
    ring = numpy.stack([numpy.arange(1.0, n - 1), numpy.arange(2.0, n), rng.uniform(0.1, 0.4, n - 2)], axis=1)
    triples = numpy.concatenate([hub, ring])
    for count in (1, 65):
        check_paths(triples, 1, n, numpy.concatenate([[0], sources_for(n, count, 3)]))


def test_components_dead_bins_duplicates_and_junk():
    n = 200
    rng = numpy.random.default_rng(21)
    a = lm.random_graph_triples(90, 300, seed=1)                     # nodes 0 .. 89
    b = lm.random_graph_triples(60, 200, seed=2)                     # nodes 100 .. 159
    b[:, :2] += 100.0
    junk_pairs = lm.random_graph_triples(n, 80, seed=3)              # cells that are no edge,
    junk_pairs[:, 2] = numpy.array([0.0, numpy.nan, -numpy.inf, -1.5, -0.0])[rng.integers(0, 5, 80)]
    again = a[rng.integers(0, 300, 60)].copy()                       # named again: the last wins
    again[:, 2] = rng.uniform(0.1, 2.0, 60)
    again[::3, :2] = again[::3, 1::-1]
    triples = numpy.concatenate([a, b, junk_pairs, again])
    triples = triples[rng.permutation(triples.shape[0])]
    sources = [0, 100, 95, 199, 150, 5, 5]
    got = check_paths(triples, 1, n, sources)
    assert not got[2].any() and not got[3].any()                     # a dead bin reaches nothing
    assert not got[0, 90:].any() and not got[1, :100].any()          # the components stay apart
    assert got[0, :90].any() and got[1, 100:160].any()


def test_an_infinite_cell_is_the_largest_double():
    """+inf is DBL_MAX after nan_to_num, as on every triple route: under 'wish' an edge of that
    length (DBL_MAX + 1.5 rounds to DBL_MAX: the path stays finite); -inf is no edge."""
    triples = numpy.array([[0.0, 1.0, 1.5], [1.0, 2.0, numpy.inf], [2.0, 3.0, 1.0], [3.0, 0.0, -numpy.inf]])
    got = check_paths(triples, 1, 4, [0, 3])
    assert got[0, 2] == im.DBL_MAX and got[0, 1] == 1.5


def test_same_bits_again_permuted_and_after_balance():
    n_bins = 300
    counts = numpy.triu(numpy.random.default_rng(6).poisson(
        30.0 * numpy.maximum(numpy.abs(numpy.subtract.outer(numpy.arange(n_bins), numpy.arange(n_bins))), 1.0)
        ** -1.5), 1).astype(numpy.float64)
    i, j = numpy.nonzero(counts)
    triples = numpy.stack([i * 1.0, j * 1.0, counts[i, j]], axis=1)   # duplicate-free
    sources = sources_for(n_bins + 1, 66, 9)
    w = lm.weights_of(triples, 1, n_bins + 1, kind="wish")
    dev = bb.DeviceTriples(triples, 1, 0)
    first = check_paths(triples, 1, n_bins + 1, sources, dev=dev, w=w)
    assert numpy.array_equal(bits(check_paths(triples, 1, n_bins + 1, sources, dev=dev, w=w)), bits(first))
    bias = dev.balance(n_bins)                                        # rebuilds the index for n_bins
    assert numpy.isfinite(bias).any()
    assert numpy.array_equal(bits(check_paths(triples, 1, n_bins + 1, sources, dev=dev, w=w)), bits(first))
    assert numpy.array_equal(dev.balance(n_bins), bias, equal_nan=True)
    dev.close()
    rng = numpy.random.default_rng(1)
    shuffled = triples[rng.permutation(triples.shape[0])]
    shuffled[::2, :2] = shuffled[::2, 1::-1]
    assert numpy.array_equal(bits(check_paths(shuffled, 1, n_bins + 1, sources, w=w)), bits(first))


def test_against_the_dense_completion():
    """Rows of `bb.shortest_paths(dense)` (blocked Floyd-Warshall): each side is a float64 sum of at
    most n - 1 positive terms and min is exact, so they agree within (n - 1) 2^-52 relative."""
    n = 500
    triples = lm.random_graph_triples(n, 2500, seed=12)
    w = lm.weights_of(triples, 1, n, kind="wish")
    dense = bb.shortest_paths(w, kind="wish")
    sources = sources_for(n, 40, 4)
    with bb.DeviceTriples(triples, 1, 0).shortest_paths(n, sources, kind="wish") as rows:
        got = rows.to_host()
    want = dense[sources]
    rel = numpy.abs(got - want) / numpy.maximum(want, 1e-300)
    print("sparse rows against the dense completion: worst relative difference %.3e (bound %.3e)"
          % (rel.max(), (n - 1) * 2.0 ** -52))
    assert ((got == 0) == (want == 0)).all()
    assert rel.max() <= (n - 1) * 2.0 ** -52


# ---- 2. the C ABI's refusals, and the handles ---------------------------------------------------
def test_argument_errors():
    triples = numpy.array([[0.0, 1.0, 2.0], [1.0, 4.0, 2.0]])
    dev = bb.DeviceTriples(triples, 1, 0)
    with pytest.raises(ValueError, match="outside"):
        dev.shortest_paths(4, [0])                     # bin 4 is outside a graph of 4 nodes
    with pytest.raises(ValueError, match="outside"):
        dev.edge_degrees(4)
    with pytest.raises(ValueError, match="source"):
        dev.shortest_paths(5, [0, 5])
    with pytest.raises(ValueError, match="source"):
        dev.shortest_paths(5, [-1])
    with pytest.raises(ValueError, match="n_sources"):
        dev.shortest_paths(5, [])
    with pytest.raises(ValueError, match="n_sources"):
        dev.shortest_paths(5, numpy.zeros(bb.GeodesicRows.MAX_SOURCES + 1, dtype=numpy.int64))
    for bad in (dict(alpha=0.0), dict(alpha=-1.0), dict(kind="distances"), dict(KRnorm=numpy.ones(4))):
        with pytest.raises(ValueError):
            dev.shortest_paths(5, [0], **bad)
    lib = _lib.load()
    out, src = _lib.c_void_p(), numpy.zeros(1, dtype=numpy.int64)
    p = src.ctypes.data_as(_lib.p_i64)
    for args in ((dev._h, 5, 7, 3.0, None, None, p, 1, out), (dev._h, 5, _lib.BB_KIND_WISH, 0.0, None, None, p, 1, out),
                 (dev._h, 0, _lib.BB_KIND_WISH, 3.0, None, None, p, 1, out),
                 (None, 5, _lib.BB_KIND_WISH, 3.0, None, None, p, 1, out),
                 (dev._h, 5, _lib.BB_KIND_WISH, 3.0, None, None, None, 1, out)):
        assert lib.bb_triples_paths(*args) == _lib.BB_ERR_INVALID and not out.value
        assert "bb_triples_paths" in _lib.last_error()
    # the handle is as good as before
    with dev.shortest_paths(5, [0, 4], kind="wish") as rows:
        assert numpy.array_equal(rows.to_host(), [[0, 2, 0, 0, 4], [4, 2, 0, 0, 0]])
        with pytest.raises(ValueError, match="outside"):
            rows.columns([5])
        with pytest.raises(ValueError, match="coef"):
            rows.place(numpy.zeros((3, 3)), numpy.zeros(2))
    dev.close()


def test_handles_close_twice_use_after_close_and_outlive_the_triples():
    triples = lm.random_graph_triples(50, 200, seed=7)
    w = lm.weights_of(triples, 1, 50, kind="wish")
    dev = bb.DeviceTriples(triples, 1, 0)
    rows = dev.shortest_paths(50, [1, 2, 3], kind="wish")
    dev.close()                                        # the rows own their memory
    dev.close()
    assert numpy.array_equal(bits(rows.to_host()), bits(lm.as_read(lm.geodesics(w, [1, 2, 3]))))
    assert rows.timing()[0] >= 0 and rows.timing()[1] >= 0
    rows.close()
    rows.close()
    for call in (rows.to_host, rows.reached, lambda: rows.columns([0]),
                 lambda: rows.place(numpy.zeros((3, 3)), numpy.zeros(3)), rows.timing):
        with pytest.raises(ValueError, match="closed"):
            call()
    assert _lib.load().bb_paths_destroy(None) == _lib.BB_OK
    assert _lib.load().bb_paths_info(None, None, None, None, None) == _lib.BB_ERR_INVALID


# ---- 3. placement -------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 5, 64, 70])
def test_place_against_the_model_sum(L):
    n = 300
    a = lm.random_graph_triples(250, 900, seed=31)     # nodes 250 .. 299 have no edge
    w = lm.weights_of(a, 1, n, kind="wish")
    rng = numpy.random.default_rng(L)
    sources = rng.integers(0, 250, L)
    sources = sources[lm.edge_degrees_of(w)[sources] > 0] if L > 1 else sources
    L = len(sources)
    coef, mu = rng.standard_normal((L, 3)), rng.uniform(0.0, 4.0, L)
    if L > 4:
        coef[2], mu[2] = 0.0, 0.0                      # a source that takes no part
    g = lm.geodesics(w, sources)
    want, placed, bound = lm.place_of(g, coef, mu)
    with bb.DeviceTriples(a, 1, 0).shortest_paths(n, sources, kind="wish") as rows:
        out = numpy.full((n, 3), 7.25)
        got, got_placed = rows.place(coef, mu, out=out)
        fresh, _ = rows.place(coef, mu)
    assert got is out and got_placed.dtype == bool and numpy.array_equal(got_placed, placed)
    assert 0 < placed.sum() < n
    assert (got[~placed] == 7.25).all() and (fresh[~placed] == 0.0).all()      # left unwritten
    err = numpy.abs(got[placed] - want[placed])
    print("L=%d: worst placement error / bound %.3f" % (L, (err / numpy.maximum(bound[placed], 1e-300)).max()))
    assert (err <= bound[placed]).all()
    assert numpy.array_equal(fresh[placed], got[placed])


# ---- 4. the landmark start ----------------------------------------------------------------------
def hic_like_triples(n, seed):
    """Counts ~ Poisson(30 d^-3) on a persistent random walk as triples at resolution 1, the
    true pair distances, and the start the existing fold test draws after them."""
    Xs = lm.chain_coords(n, seed)
    Ds = lm.pair_distances(Xs)
    r = numpy.random.default_rng(100 + seed)
    lam = 30.0 * numpy.maximum(Ds, 1e-9) ** -3.0
    numpy.fill_diagonal(lam, 0)
    C = numpy.triu(r.poisson(lam), 1).astype(float)
    X0 = r.standard_normal((n, 3))
    i, j = numpy.nonzero(C)
    return numpy.stack([i * 1.0, j * 1.0, C[i, j]], axis=1), Ds, X0, C + C.T


@pytest.fixture(scope="module")
def chain():
    return hic_like_triples(400, 1)


def test_landmark_start_is_place_of_its_own_landmarks(chain):
    triples, _, _, _ = chain
    # a second, smaller component (bins 410 .. 449) and dead bins around it: landmarks that are
    # dropped, bins that are not placed
    i = numpy.arange(410.0, 449.0)
    t = numpy.concatenate([triples, numpy.stack([i, i + 1, numpy.full(i.size, 5.0)], axis=1)])
    n_bins = 459
    start, info = bb.landmark_start(t, 1, n_bins, n_landmarks=16, seed=3, return_info=True)
    assert start.shape == (n_bins + 1, 3) and start.dtype == numpy.float64
    w = lm.weights_of(t, 1, n_bins + 1, kind="counts", alpha=3.0)
    live = numpy.flatnonzero(lm.edge_degrees_of(w) > 0)
    assert numpy.array_equal(info.landmarks_, lm.landmarks_of(live, 16))
    g = lm.geodesics(w, info.landmarks_)
    main = int(numpy.argmax((~numpy.isinf(g)).sum(axis=1)))
    assert numpy.array_equal(info.kept_, ~numpy.isinf(g[main, info.landmarks_])) and not info.kept_.all()
    assert numpy.array_equal(info.placed_, ~numpy.isinf(g[main]))
    assert not info.placed_[400:].any() and info.placed_.sum() >= 390
    assert info.unreachable_ == int(numpy.isinf(g).sum()) and 1 <= info.sweeps_ <= n_bins + 1
    default = numpy.random.default_rng(3).standard_normal((n_bins + 1, 3))
    assert numpy.array_equal(start[~info.placed_], default[~info.placed_])
    dev = bb.DeviceTriples(t, 1, 0)
    with dev.shortest_paths(n_bins + 1, info.landmarks_) as rows:
        G = rows.columns(info.landmarks_)
        coef, mu = numpy.zeros((16, 3)), numpy.zeros(16)
        coef[info.kept_], mu[info.kept_] = bb.landmark_coefficients(G[numpy.ix_(info.kept_, info.kept_)])
        want, placed = rows.place(coef, mu, out=default.copy())
    assert numpy.array_equal(placed, info.placed_) and numpy.array_equal(bits(start), bits(want))
    # an open DeviceTriples gives the same, and stays open
    assert numpy.array_equal(bits(bb.landmark_start(dev, 1, n_bins, n_landmarks=16, seed=3)), bits(start))
    assert dev.pairs(n_bins) > 0
    dev.close()
    # and the whole rule agrees with the model to the placement bound
    m_start, m_lm, m_kept, m_placed, m_coef, m_mu, m_g = lm.landmark_start_of(w, 16, 3)
    assert numpy.array_equal(m_placed, info.placed_)
    scale = numpy.abs(m_start[m_placed]).max()
    assert numpy.abs(start - m_start).max() <= 1e-9 * scale


def _same_fit(a, b):
    return numpy.array_equal(a.structure_, b.structure_) and numpy.array_equal(a.stress_, b.stress_)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_fit_triples_with_the_landmark_init_is_the_fit_from_landmark_start(chain, dtype):
    import scipy.sparse
    triples, _, _, C = chain
    n_bins = 399
    kw = dict(n_iter=5, dtype=dtype, alpha=3.0, kind="counts", degree_steps=True, seed=2)
    make = lambda **more: bb.StructureSolver(init=("landmark", 16), **dict(kw, **more))
    plain = lambda **more: bb.StructureSolver(**dict(kw, **more))
    start, info = bb.landmark_start(triples, 1, n_bins, n_landmarks=16, seed=2, return_info=True)
    got = make().fit_triples(triples, 1, n_bins)
    assert _same_fit(got, plain().fit_triples(triples, 1, n_bins, init=start))
    assert numpy.array_equal(got.landmarks_, info.landmarks_)
    assert numpy.array_equal(got.landmark_placed_, info.placed_)
    assert not _same_fit(got, plain().fit_triples(triples, 1, n_bins))
    # an open DeviceTriples
    dev = bb.DeviceTriples(triples, 1, 0)
    assert _same_fit(make().fit_triples(dev, 1, n_bins), got)
    dev.close()
    # the default number of landmarks
    start64 = bb.landmark_start(triples, 1, n_bins, seed=2)
    assert _same_fit(bb.StructureSolver(init="landmark", **kw).fit_triples(triples, 1, n_bins),
                     plain().fit_triples(triples, 1, n_bins, init=start64))
    # several members on one GPU: the start is computed once, the fit is the group's
    assert _same_fit(make(devices=[0, 0]).fit_triples(triples, 1, n_bins),
                     plain(devices=[0, 0]).fit_triples(triples, 1, n_bins, init=start))
    # balance=True: the start uses the bias the fit uses
    bal = bb.balance_triples(triples, 1, n_bins)
    bal_start = bb.landmark_start(triples, 1, n_bins, n_landmarks=16, seed=2, KRnorm=bal.bias,
                                  KRexpected=numpy.ones(n_bins))
    assert not numpy.array_equal(bal_start, start)
    assert _same_fit(make().fit_triples(triples, 1, n_bins, balance=True),
                     plain().fit_triples(triples, 1, n_bins, balance=True, init=bal_start))
    # explicit KR vectors
    assert _same_fit(make().fit_triples(triples, 1, n_bins, KRnorm=bal.bias, KRexpected=numpy.ones(n_bins)),
                     plain().fit_triples(triples, 1, n_bins, KRnorm=bal.bias, KRexpected=numpy.ones(n_bins),
                                         init=bal_start))
    # scipy.sparse input: the COO entries are the triples at resolution 1
    sp = scipy.sparse.coo_matrix(numpy.triu(C, 1))
    from_sparse = make().fit(sp)
    assert _same_fit(from_sparse, plain().fit(sp, init=start))
    assert numpy.array_equal(from_sparse.landmarks_, info.landmarks_)
    assert _same_fit(from_sparse, got)


def test_too_disconnected_a_map_is_refused():
    pairs = numpy.array([[0.0, 1.0, 3.0], [4.0, 5.0, 3.0], [8.0, 9.0, 3.0], [12.0, 13.0, 3.0], [13.0, 14.0, 2.0]])
    with pytest.raises(ValueError, match="too disconnected for a landmark start"):
        bb.landmark_start(pairs, 1, 20, n_landmarks=8)          # the largest component holds 3
    with pytest.raises(ValueError, match="too disconnected for a landmark start"):
        bb.landmark_start(pairs[:1], 1, 20, n_landmarks=8)      # two live bins
    with pytest.raises(ValueError, match="too disconnected for a landmark start"):
        bb.StructureSolver(init=("landmark", 8), n_iter=1).fit_triples(pairs, 1, 20)


# ---- 5. it does what it is for ------------------------------------------------------------------
def test_the_landmark_start_holds_the_global_fold_of_a_sparse_map(chain):
    """The chain of tests/test_gpu_shortest_paths.py's fold test (n = 400, seed 1, the same
    counts) as triples, 16 landmarks, degree_steps, float64; its thresholds.  A numpy / scipy
    float64 model gives 0.958 for the start, 0.957 after 100 iterations and 0.045 for the random
    start (after 300)."""
    import scipy.stats
    triples, Ds, X0, _ = chain
    n = 400
    iu = numpy.triu_indices(n, 1)
    rho = lambda X: float(scipy.stats.spearmanr(lm.pair_distances(X)[iu], Ds[iu])[0])
    kw = dict(dtype="float64", kind="counts", alpha=3.0, degree_steps=True)
    start = bb.landmark_start(triples, 1, n - 1, n_landmarks=16)
    fitted = bb.StructureSolver(n_iter=100, init=("landmark", 16), **kw).fit_triples(triples, 1, n - 1)
    random = bb.StructureSolver(n_iter=300, **kw).fit_triples(triples, 1, n - 1, init=X0)
    r_start, r_fit, r_random = rho(start), rho(fitted.structure_), rho(random.structure_)
    print("stored pairs %.1f %%, Spearman: landmark start %.3f, after 100 iterations %.3f, random "
          "start %.3f" % (100.0 * triples.shape[0] / iu[0].size, r_start, r_fit, r_random))
    assert fitted.landmark_placed_.all() and fitted.landmarks_.shape == (16,)
    assert r_start >= 0.7
    assert r_fit >= 0.7
    assert r_random <= 0.3
