"""GPU: pooling a map to a coarser resolution (docs/SPEC.md 2.12) -- `ContactMap.coarsen`,
`DeviceTriples.coarsen` / `.to_host`, `coarsen_triples` -- bit for bit against the numpy model of
tests/_coarsen_model.py, whose order of summation is the definition's (tests/test_coarsen_cpu.py
shows that another order gives other bits on the non-integer maps used here), and the pixel-list
route bit for bit against the dense one.  Sizes sit around the constants of bb_coarsen.hip, named
below.  No tolerance anywhere: every comparison is of bit patterns."""
import numpy
import pytest

import blueberry_amd as bb
from blueberry_amd import _lib
from tests import _coarsen_model as cm
from tests._util import same_bits

pytestmark = pytest.mark.gpu

# the constants of bb_coarsen.hip
CO_ROWS = 8          # kCoRows: fine rows of a step; a factor above it takes several row steps
CO_TILE = 512        # kCoTile: fine columns of a step; a factor above it walks its column in tiles
CO_COLS = 256        # kCoCols: coarse columns of a workgroup, at most (factors 1 and 2)
CO_CHUNK = 2048      # kCoChunk: pooled columns whose accumulators the pixel-list kernel holds
TB_SEG = 1024        # kTbSeg of the index the pixel-list kernel reads (bb_triples.h)
RES = 1000

N_BINS = [1, 2, 3, 63, 64, 65, 127, 128, 129, 257, 1000, 1025]
FACTORS = [1, 2, 3, 5, 7, 10, 16, 64, 100]        # and n_bins, n_bins + 1


def pool_and_check(cmap, M, n, k, how):
    out = cmap.coarsen(k, how)
    want = cm.pooled(M, n, k, how)
    got = out.matrix
    assert got.shape == want.shape, (n, k, how)
    bad = numpy.argwhere(got.view(numpy.uint64) != want.view(numpy.uint64))
    assert bad.shape[0] == 0, (n, k, how, bad[:4], got[tuple(bad[0])], want[tuple(bad[0])])
    return out


# ---- 1. dense, bit for bit against the model -----------------------------------------------------
@pytest.mark.parametrize("n", N_BINS)
@pytest.mark.parametrize("kind", ["integer", "wide"])
def test_dense_equals_the_model(n, kind):
    """Every n_bins with every factor -- each factor meets exact and ragged n_bins -- both `how`."""
    for k in FACTORS + [n, n + 1]:
        M = cm.integer_map(n, 100 + n) if kind == "integer" else cm.wide_map(n, cm.wide_seed(n, k))
        cmap = bb.ContactMap.from_matrix(M, resolution=RES)
        for how in ("sum", "mean"):
            pool_and_check(cmap, M, n, k, how)


@pytest.mark.parametrize("n,k", cm.ORDER_CASES)
def test_dense_on_the_maps_where_the_order_is_shown_to_matter(n, k):
    M = cm.wide_map(n, cm.wide_seed(n, k))
    pool_and_check(bb.ContactMap.from_matrix(M), M, n, k, "sum")


EDGES = ([(n, k) for k in (CO_ROWS - 1, CO_ROWS, CO_ROWS + 1) for n in (8 * k, 8 * k + 1, 515)]
         + [(n, k) for k in (CO_TILE - 1, CO_TILE, CO_TILE + 1) for n in (k - 1, k, k + 1, 2 * k + 3)]
         # factor 1: CO_COLS pooled = fine columns per workgroup; factor 2: CO_COLS pooled, CO_TILE fine
         + [(n, 1) for n in (CO_COLS - 1, CO_COLS, CO_COLS + 1, 2 * CO_COLS + 1)]
         + [(n, 2) for n in (CO_TILE - 1, CO_TILE, CO_TILE + 1, CO_TILE + 2, 2 * CO_TILE + 1)]
         # factor 3 and 5: 170 and 102 pooled columns per workgroup = 510 fine columns
         + [(n, k) for k in (3, 5) for n in (509, 510, 511, 512, 1021)])


@pytest.mark.parametrize("n,k", EDGES)
def test_dense_around_the_kernel_constants(n, k):
    M = cm.wide_map(n, cm.wide_seed(n, k))
    cmap = bb.ContactMap.from_matrix(M)
    for how in ("sum", "mean"):
        pool_and_check(cmap, M, n, k, how)


# ---- 2. what the result looks like ---------------------------------------------------------------
@pytest.mark.parametrize("n,k", [(129, 10), (1025, 7), (257, 258)])
def test_result_is_symmetric_with_a_zero_padding(n, k):
    M = cm.wide_map(n, 5)
    got = bb.ContactMap.from_matrix(M).coarsen(k).matrix
    assert same_bits(got, numpy.ascontiguousarray(got.T))
    assert not got[-1].view(numpy.uint64).any() and not got[:, -1].view(numpy.uint64).any()


@pytest.mark.parametrize("n", [1, 64, 257, 1025])
def test_factor_one_is_the_leading_block_mirrored_from_the_upper_triangle(n):
    M = cm.wide_map(n, 11)
    M[n // 2, 0] = 123.0                               # below the diagonal: never read
    got = bb.ContactMap.from_matrix(M).coarsen(1).matrix
    U = numpy.triu(M[:n, :n])
    want = numpy.zeros((n + 1, n + 1))
    want[:n, :n] = U + numpy.triu(U, 1).T
    assert same_bits(got, want)


def test_only_the_upper_triangle_is_read():
    n, k = 257, 5
    M = cm.wide_map(n, 3)
    A = M.copy()
    A[numpy.tril_indices(n + 1, -1)] = numpy.random.default_rng(0).random((n + 1) * n // 2) * 1e6
    A[n // 3, n // 4] = numpy.nan
    assert same_bits(bb.ContactMap.from_matrix(A).coarsen(k).matrix, cm.pooled(M, n, k))


@pytest.mark.parametrize("n,k,cell", [(257, 5, (100, 203)), (257, 5, (101, 101)), (129, 16, (3, 128)),
                                      (1025, 100, (0, 1024))])
def test_a_nan_poisons_exactly_one_pooled_cell(n, k, cell):
    M = cm.integer_map(n, 9)
    clean = cm.pooled(M, n, k)
    i, j = cell
    for poison in (numpy.nan, numpy.inf):
        A = M.copy()
        A[i, j] = A[j, i] = poison
        got = bb.ContactMap.from_matrix(A).coarsen(k).matrix
        hit = numpy.zeros(got.shape, dtype=bool)
        hit[i // k, j // k] = hit[j // k, i // k] = True
        assert same_bits(got[~hit], clean[~hit])
        assert (numpy.isnan(got[hit]) if poison != poison else numpy.isinf(got[hit])).all()
        assert same_bits(got, cm.pooled(A, n, k))


# ---- 3. the source -------------------------------------------------------------------------------
def test_the_source_stays_as_it_is_and_resident():
    n, k = 257, 3
    M = cm.wide_map(n, 21)
    t = cm.triples_of(M, n, RES)
    src = bb.ContactMap.from_triples(t, RES, n)
    view = src.matrix
    before = numpy.array(view)
    out = src.coarsen(k)
    assert src.is_resident and out.is_resident
    assert src.matrix is view                                   # the host copy handed out stays valid
    assert same_bits(src.to_host(), before)
    Mt = before.copy()
    assert same_bits(out.matrix, cm.pooled(Mt, n, k))


def test_a_filtered_map_is_refused():
    n = 64
    M = cm.integer_map(n, 2)
    M[5, :] = M[:, 5] = 0.0
    for keep_stale in (False, True):
        cmap = bb.ContactMap.from_matrix(M)
        cmap.filter(0, keep_stale=keep_stale)
        with pytest.raises(ValueError):
            cmap.coarsen(2)
        # the library's own check, past the Python one
        dst = bb.datatypes._DeviceMatrix(n // 2 + 1, 0)
        rc = cmap._dev._status("coarsen", n, 2, _lib.BB_COARSEN_SUM, dst._open())
        assert rc == _lib.BB_ERR_INVALID and "filtered" in _lib.last_error()
        dst.close()


def test_library_argument_checks():
    n = 10
    src = bb.datatypes._DeviceMatrix(n + 1, 0)
    dst, small = bb.datatypes._DeviceMatrix(6, 0), bb.datatypes._DeviceMatrix(5, 0)
    bad = [(n, 0, 0, dst), (n, 2, 7, dst), (n, 2, 0, small), (n, 2, 0, src), (-1, 2, 0, dst)]
    for nb, k, how, d in bad:
        assert src._status("coarsen", nb, k, how, d._open()) == _lib.BB_ERR_INVALID, (nb, k, how)
    assert src._status("coarsen", n, 2, 0, None) == _lib.BB_ERR_INVALID
    assert src._status("coarsen", n, 2, 0, dst._open()) == _lib.BB_OK
    tr = bb.DeviceTriples(numpy.array([[0.0, 1000.0, 2.0]]), RES, 0)
    h = _lib.c_void_p()
    assert tr._status("coarsen", n, 0, 0, h) == _lib.BB_ERR_INVALID and not h
    assert tr._status("coarsen", n, 2, 5, h) == _lib.BB_ERR_INVALID and not h
    assert tr._status("coarsen", n, 2 ** 31, 0, h) == _lib.BB_ERR_INVALID and not h      # R x factor
    for x in (src, dst, small, tr):
        x.close()


def test_a_host_authoritative_map_is_uploaded_first():
    n, k = 129, 7
    M = cm.wide_map(n, 4)
    cmap = bb.ContactMap.from_matrix(M)
    assert not cmap.is_resident
    out = cmap.coarsen(k, "mean")
    assert cmap.is_resident and same_bits(out.matrix, cm.pooled(M, n, k, "mean"))
    host = cmap.host_matrix()                       # back to the host, changed there
    host[0, 1] = host[1, 0] = 77.0
    assert not cmap.is_resident
    assert same_bits(cmap.coarsen(k).matrix, cm.pooled(host, n, k))


# ---- 4. the result's state -----------------------------------------------------------------------
def test_the_result_is_a_contact_map_of_the_coarse_resolution():
    n, k = 130, 4
    M = cm.integer_map(n, 6) + 1.0
    M[n, :] = M[:, n] = 0.0
    regions = numpy.array([0.0, 1000.0, 3000.0, 4500.0, 8000.0, 129000.0])
    src = bb.ContactMap.from_matrix(M, resolution=RES, celltype="GM", chromosome=7,
                                    KRnorm=numpy.ones(n), KRexpected=numpy.ones(n))
    src.regions = regions
    src.balance(max_iter=3)
    src.expected()
    out = src.coarsen(k)
    nc = 33
    assert (out.resolution, out.n_bins, out.celltype, out.chromosome, out.device) == (4000, nc, "GM", 7, src.device)
    assert out.shape == (nc + 1, nc + 1) and out.is_resident
    assert numpy.array_equal(out.regions, [0.0, 4000.0, 8000.0, 128000.0])
    assert out._KRnorm is None and out._KRexpected is None
    for name in ("balance_iterations_", "balance_masked_", "expected_sums_", "expected_counts_"):
        assert not hasattr(out, name)
    assert src._KRnorm is not None and src.n_bins == n and src.resolution == RES
    with pytest.raises(ValueError, match="KRnorm"):
        out.normalize()
    # and it feeds what a ContactMap feeds
    bias = out.balance(max_iter=20)
    assert bias.shape == (nc,) and numpy.isfinite(bias).all()
    assert out.expected().shape == (nc,)
    s = bb.StructureSolver(n_iter=5, dtype="float64").fit(out)
    assert s.structure_.shape == (nc + 1, 3) and numpy.isfinite(s.structure_).all()
    again = out.coarsen(2)                          # a pooled map pools again
    assert again.n_bins == 17 and again.resolution == 8000
    out.correlation()
    assert out.matrix.shape == (nc + 1, nc + 1)


def test_pooling_twice_equals_pooling_once_on_integer_maps():
    n = 240
    M = cm.integer_map(n, 8)
    cmap = bb.ContactMap.from_matrix(M)
    assert same_bits(cmap.coarsen(4).coarsen(3).matrix, cmap.coarsen(12).matrix)


# ---- 5. the pixel list equals the dense route ----------------------------------------------------
def dense_route(t, n, k, how):
    with_matrix = bb.ContactMap.from_triples(t, RES, n)
    return with_matrix.coarsen(k, how).matrix


def check_pixel_list(t, n, k, how="sum", model=True):
    pooled, nc = bb.coarsen_triples(t, RES, n, k, how)
    assert nc == cm.n_coarse(n, k) and pooled.shape[1] == 3 and pooled.flags.c_contiguous
    R = RES * k
    I, J = pooled[:, 0] / R, pooled[:, 1] / R
    assert numpy.array_equal(I, I.astype(numpy.int64)) and (I <= J).all() and (J < max(nc, 1)).all()
    key = I * max(nc, 1) + J
    assert (numpy.diff(key) > 0).all()                          # canonical order, every cell once
    want = dense_route(t, n, k, how)
    got = bb.ContactMap.from_triples(pooled, R, nc).matrix
    assert same_bits(got[:nc, :nc], want[:nc, :nc]), (n, k, how)
    if model:
        want_t, _ = cm.pooled_triples(t, RES, n, k, how)
        assert same_bits(pooled, want_t), (n, k, how)
    return pooled


def messy_list(n, seed):
    """Duplicates (the last wins), stored zeros, diagonal cells, either orientation, positions
    anywhere inside their bins, and triples that touch bin n (never read)."""
    r = numpy.random.default_rng(seed)
    M = cm.wide_map(n, seed)
    t = cm.triples_of(M, n, RES, keep_zeros=0.3, seed=seed)
    t = t[r.random(t.shape[0]) < 0.5]
    dup = t[r.integers(0, max(t.shape[0], 1), t.shape[0] // 4)].copy()
    dup[:, 2] = r.uniform(0.5, 1.0, dup.shape[0]) * 2.0 ** r.integers(-20, 21, dup.shape[0])
    edge = numpy.stack([r.integers(0, n + 1, 9) * float(RES), numpy.full(9, n * float(RES)), numpy.full(9, 5.0)], 1)
    t = numpy.concatenate([t, dup, edge])
    t = t[r.permutation(t.shape[0])]
    flip = r.random(t.shape[0]) < 0.5
    t[flip, 0], t[flip, 1] = t[flip, 1].copy(), t[flip, 0].copy()
    t[:, :2] += r.integers(0, RES, (t.shape[0], 2))
    return t


@pytest.mark.parametrize("n,k", [(1, 1), (2, 3), (3, 2), (64, 2), (65, 16), (129, 10), (257, 1), (257, 5),
                                 (257, 257), (257, 300), (1000, 7), (1025, 64)])
def test_pixel_list_equals_dense_on_messy_lists(n, k):
    t = messy_list(n, 31 * n + k)
    for how in ("sum", "mean"):
        check_pixel_list(t, n, k, how)


def test_pixel_list_memory_orders_and_permutations_give_the_same_bits():
    n, k = 257, 5
    t = cm.triples_of(cm.wide_map(n, 77), n, RES, keep_zeros=0.2, seed=1)     # duplicate-free
    want = check_pixel_list(t, n, k)
    r = numpy.random.default_rng(5)
    for trial in range(3):
        p = t[r.permutation(t.shape[0])]
        flip = r.random(p.shape[0]) < 0.5
        p[flip, 0], p[flip, 1] = p[flip, 1].copy(), p[flip, 0].copy()
        for arr in (p, numpy.asfortranarray(p), numpy.repeat(p, 2, axis=0)[::2]):
            assert same_bits(bb.coarsen_triples(arr, RES, n, k)[0], want)


def test_an_empty_list_pools_to_an_empty_list():
    pooled, nc = bb.coarsen_triples(numpy.zeros((0, 3)), RES, 100, 7)
    assert pooled.shape == (0, 3) and nc == 15
    only_edge = numpy.array([[100.0 * RES, 3.0 * RES, 2.0]])     # touches bin n_bins alone
    assert bb.coarsen_triples(only_edge, RES, 100, 7)[0].shape == (0, 3)
    assert bb.coarsen_triples(numpy.zeros((0, 3)), RES, 0, 3) [1] == 0


def sparse_list(n, seed, per_bin=6, hub=None):
    """A duplicate-free sparse list over n bins: a band of 2, `per_bin` random far cells per bin,
    and every cell of row `hub`."""
    r = numpy.random.default_rng(seed)
    i = numpy.concatenate([numpy.repeat(numpy.arange(n), 3), r.integers(0, n, per_bin * n)])
    j = numpy.concatenate([numpy.repeat(numpy.arange(n), 3) + numpy.tile(numpy.arange(3), n),
                           r.integers(0, n, per_bin * n)])
    if hub is not None:
        i = numpy.concatenate([i, numpy.full(n, hub)])
        j = numpy.concatenate([j, numpy.arange(n)])
    ok = j < n
    key = numpy.unique(numpy.minimum(i, j)[ok] * n + numpy.maximum(i, j)[ok])
    v = r.uniform(0.5, 1.0, key.shape[0]) * 2.0 ** r.integers(-20, 21, key.shape[0])
    t = numpy.stack([(key // n) * float(RES), (key % n) * float(RES), v], axis=1)
    return t[r.permutation(t.shape[0])]


@pytest.mark.parametrize("k", [1, 3, 100])
def test_a_hub_row_longer_than_a_segment(k):
    n = TB_SEG + 300
    t = sparse_list(n, 3, hub=5)
    assert (numpy.minimum(t[:, 0], t[:, 1]) == 5 * RES).sum() + 5 > TB_SEG
    check_pixel_list(t, n, k)


@pytest.mark.parametrize("n,k", [(CO_CHUNK - 1, 1), (CO_CHUNK, 1), (CO_CHUNK + 1, 1), (2 * CO_CHUNK + 3, 2),
                                 (2 * CO_CHUNK + 3, 1)])
def test_pooled_rows_wider_than_one_column_chunk(n, k):
    """nc around and beyond kCoChunk: a pooled row is walked in column chunks (rows that start in
    the first chunk and rows that start in the second)."""
    t = sparse_list(n, n + k, per_bin=4, hub=7)
    nc = cm.n_coarse(n, k)
    pooled = check_pixel_list(t, n, k)
    if nc > CO_CHUNK:
        J = pooled[:, 1] / (RES * k)
        I = pooled[:, 0] / (RES * k)
        assert ((J >= CO_CHUNK) & (I < CO_CHUNK)).any() and (I >= CO_CHUNK).any()


# ---- 6. the resident handle ----------------------------------------------------------------------
def test_the_resident_pooled_handle_equals_the_host_route_and_feeds_the_consumers():
    n, k = 400, 4
    nc = 100
    t = sparse_list(n, 12, per_bin=30)
    t[:, 2] = numpy.random.default_rng(1).integers(1, 30, t.shape[0])      # counts
    host, nc_host = bb.coarsen_triples(t, RES, n, k)
    dev = bb.DeviceTriples(t, RES, 0)
    assert same_bits(dev.to_host(), t)
    assert same_bits(bb.DeviceTriples(numpy.asfortranarray(t), RES, 0).to_host(), t)
    pooled = dev.coarsen(n, k)
    assert isinstance(pooled, bb.DeviceTriples) and pooled.is_triples
    assert (pooled.resolution, pooled.n_bins_, pooled.device, pooled.n) == (RES * k, nc, 0, host.shape[0])
    assert nc_host == nc and same_bits(pooled.to_host(), host)
    assert same_bits(dev.to_host(), t) and dev.pairs(n) == t.shape[0]
    copy = bb.DeviceTriples(host, RES * k, 0)
    # fit_triples: the same bits from the resident handle as from its host copy
    fits = []
    for src in (pooled, host):
        s = bb.StructureSolver(n_iter=20, dtype="float64", seed=3)
        s.fit_triples(src, RES * k, nc)
        fits.append((s.structure_, s.stress_))
    assert same_bits(fits[0][0], fits[1][0]) and same_bits(fits[0][1], fits[1][1])
    assert numpy.isfinite(fits[0][0]).all()
    # balance, expected, significance, landmark_start: as from the copy
    assert same_bits(pooled.balance(nc, max_iter=10), copy.balance(nc, max_iter=10))
    assert same_bits(pooled.expected(nc), copy.expected(nc))
    sig_a, sig_b = pooled.significance(nc, n_bins=10), copy.significance(nc, n_bins=10)
    assert same_bits(sig_a.map, sig_b.map) and sig_a.map.shape[0] > 0
    assert same_bits(bb.landmark_start(pooled, RES * k, nc, n_landmarks=8),
                     bb.landmark_start(copy, RES * k, nc, n_landmarks=8))
    assert same_bits(pooled.coarsen(nc, 5).to_host(), bb.coarsen_triples(host, RES * k, nc, 5)[0])
    for x in (dev, pooled, copy):
        x.close()


def test_two_calls_give_the_same_bits():
    n, k = 1025, 10
    M = cm.wide_map(n, 1)
    cmap = bb.ContactMap.from_matrix(M)
    a = cmap.coarsen(k).matrix
    for _ in range(3):
        assert same_bits(cmap.coarsen(k).matrix, a)
    t = messy_list(257, 2)
    b = bb.coarsen_triples(t, RES, 257, 5, "mean")[0]
    with bb.DeviceTriples(t, RES, 0) as dev:
        for _ in range(3):
            with dev.coarsen(257, 5, "mean") as p:
                assert same_bits(p.to_host(), b)


# ---- 7. handle lifetimes -------------------------------------------------------------------------
def test_the_result_outlives_its_source_and_closes_twice():
    n, k = 129, 3
    M = cm.wide_map(n, 13)
    t = cm.triples_of(M, n, RES)
    src = bb.ContactMap.from_triples(t, RES, n)
    out = src.coarsen(k)
    src._dev.close()
    src._dev.close()
    assert same_bits(out.matrix, cm.pooled(bb.ContactMap.from_triples(t, RES, n).matrix, n, k))
    dev = bb.DeviceTriples(t, RES, 0)
    pooled = dev.coarsen(n, k)
    dev.close()
    dev.close()
    want, _ = cm.pooled_triples(t, RES, n, k)
    assert same_bits(pooled.to_host(), want)
    assert same_bits(pooled.coarsen(43, 2).to_host(), cm.pooled_triples(want, RES * k, 43, 2)[0])
    pooled.close()
    pooled.close()
    for call in (lambda: pooled.to_host(), lambda: pooled.coarsen(43, 2), lambda: dev.coarsen(n, k),
                 lambda: dev.to_host()):
        with pytest.raises(ValueError, match="closed"):
            call()
