"""GPU: landmark constraints inside the fit (docs/SPEC.md 2.5.5; `bb_solver_set_anchors`,
`bb_solver_anchor_*`, `StructureSolver(init=('landmark', n, landmark_weight))`).

The reference is tests/_anchor_model.py, numpy float64 written from the specification, never the
library.  Maps are 'wish' triples (the counts of tests/_anchor_model.hic_like_triples turned into
distances by numpy), so that no device pow() stands between the model's graph and the device's:
the geodesics are then scipy's bits (tests/test_gpu_landmark.py) and the model's anchors are the
device's, value for value.

Sizes.  The node kernel owns 256 nodes per workgroup, the landmark side 1,024 per chunk, the rows
are padded to n_pad, the sources of a bb_paths to 64: node counts one below, at and one above the
block width vw of each dtype and 2 vw + 1 (1,025 in fp32: two chunks), kept rows 4, 63, 64, 65 and
130.  Every map has dead bins, a second component that two dropped sources lie in (its nodes are
unreachable: no term), and two kept landmarks that are also a stored pair."""
import ctypes

import numpy
import pytest

import blueberry_amd as bb
from blueberry_amd import _lib
from blueberry_amd.solver import HipEngine, layout_info
from tests import _anchor_model as am
from tests import _input_model as im
from tests import _landmark_model as lm
from tests._util import bits

pytestmark = pytest.mark.gpu

TOL = {"float64": 1e-12, "float32": 1e-5}              # SPEC 4
VW = {d: layout_info(100, d)["vw"] for d in TOL}       # the block width of maps this small


def wish_map(n, seed):
    """'wish' triples over n nodes: the chain of hic_like_triples over the first n - 24, three
    dead bins inside it, then 4 dead bins, a path of 16 nodes (a second component), 4 dead bins."""
    m = n - 24
    t = am.hic_like_triples(m, seed)[0]
    t[:, 2] = t[:, 2] ** (-1.0 / 3.0)
    dead = numpy.random.default_rng(seed).choice(numpy.arange(5, m - 5), 3, replace=False)
    t = t[~numpy.isin(t[:, 0], dead) & ~numpy.isin(t[:, 1], dead)]
    i = numpy.arange(m + 4.0, m + 19.0)
    return numpy.concatenate([t, numpy.stack([i, i + 1, numpy.full(i.size, 0.7)], axis=1)]), dead, m


class Case(object):
    """One map, its sources (`count` kept ones in the main component, two dropped ones in the
    second) and the model's view of both for a `dtype` run."""

    def __init__(self, dtype, n, count, seed=1):
        self.dtype, self.n = dtype, n
        self.triples, self.dead, m = wish_map(n, seed)
        self.w64 = lm.weights_of(self.triples, 1, n, kind="wish")
        self.w = im.matrix_of("triples", n, dtype, kind="wish", triples=self.triples, resolution=1)
        rng = numpy.random.default_rng(seed + count)
        main = numpy.flatnonzero(~numpy.isinf(lm.geodesics(self.w64, [0])[0]))
        pair = next(int(v) for v in main if v + 1 in main and self.w64[v, v + 1] > 0 and v > 10)
        rest = numpy.setdiff1d(main, [pair, pair + 1])
        kept_nodes = numpy.concatenate([[pair, pair + 1], rng.choice(rest, count - 2, replace=False)])
        src = numpy.concatenate([kept_nodes, [m + 6, m + 12]])
        order = rng.permutation(src.size)
        self.sources = src[order]
        self.kept = numpy.isin(self.sources, kept_nodes)
        self.g = lm.geodesics(self.w64, self.sources)
        self.A, self.nodes = am.anchors_of(self.g, self.sources, self.kept, dtype)
        assert self.A[list(self.nodes).index(pair), pair + 1] > 0 and self.w[pair, pair + 1] > 0
        self.free = numpy.flatnonzero(~(self.A > 0).any(axis=0) & ~numpy.isin(numpy.arange(n), self.nodes))
        assert self.free.size >= 27 and set(self.dead) <= set(self.free)     # dead bins, the second component
        x = 3.0 * rng.standard_normal((n, 3))
        self.X = x.astype(dtype).astype(numpy.float64)
        self.scale = rng.uniform(0.5, 2.0, n).astype(dtype).astype(numpy.float64)

    def engine(self, lam, q=0, anchors=True):
        """An engine holding the map (and the anchors: the paths are destroyed before it is used)."""
        dev = bb.DeviceTriples(self.triples, 1, 0)
        try:
            e = HipEngine(self.n, self.dtype, tiles=dev.tiles(self.n, self.dtype))
            e.set_wish_triples(dev, "wish", 3.0)
            e.set_weight_power(q)
            if anchors:
                with dev.shortest_paths(self.n, self.sources, kind="wish") as rows:
                    assert numpy.array_equal(bits(rows.to_host()), bits(lm.as_read(self.g)))
                    e.set_anchors(rows, self.kept, lam)
        finally:
            dev.close()
        return e


_cases = {}


def case_of(dtype, n, count):
    key = (dtype, n, count)
    if key not in _cases:
        _cases[key] = Case(dtype, n, count)
    return _cases[key]


def shapes(dtype):
    vw = VW[dtype]
    return [(vw - 1, 63, 1), (vw, 64, 2), (vw + 1, 65, 0), (2 * vw + 1, 130, 1), (vw + 1, 4, 2), (2 * vw + 1, 64, 0)]


EXCHANGE_CASES = [(d,) + s for d in TOL for s in shapes(d)]


@pytest.mark.parametrize("dtype,n,count,q", EXCHANGE_CASES)
def test_exchange_buffer_sums_and_stress_against_the_model(dtype, n, count, q):
    c, lam = case_of(dtype, n, count), 0.3
    terms = am.Terms(c.w, c.A, c.nodes, lam)
    S, Sa, g = am.objective(c.X, terms, q, dtype)
    want = c.scale[:, None] * g
    e = c.engine(lam, q)
    try:
        n_pad = e.layout()["n_pad"]
        assert e.anchored and e.anchor_info()[:2] == (count, int((c.A > 0).sum()))
        assert e.anchor_info()[2] >= count * n_pad * (4 if dtype == "float32" else 8)
        e.set_bin_steps(c.scale)
        e.set_coords(c.X)
        e.grad()
        ex = e.read_exchange()
        got = ex[:3 * n].reshape(n, 3)
        err = numpy.abs(got - want).max() / numpy.abs(want).max()
        print("%s n %d L' %d q %d: gradient %.2e, stress %.2e (relative)"
              % (dtype, n, count, q, err, abs(ex[-2] + ex[-1] - S) / S))
        assert err <= TOL[dtype]
        assert abs(ex[-2] + ex[-1] - S) <= TOL[dtype] * S
        assert not ex[3 * n:3 * n_pad].any()                               # the padding rows: exactly 0
        e.set_coords(c.X)                                                  # (drops the pending gradient)
        assert abs(e.stress() - S) <= TOL[dtype] * S
        assert abs(e.anchor_stress() - Sa) <= TOL[dtype] * Sa
        # the step quantities: float64 sums in a fixed order
        s_all, s_anchor = am.sums_of(terms, q)
        n_terms = (c.A > 0).sum(axis=0).astype(float)
        n_terms[c.nodes] += (c.A > 0).sum(axis=1)
        sums = e.anchor_sums()
        assert (numpy.abs(sums - s_anchor) <= (n_terms + 1) * 2.0 ** -52 * s_anchor).all()
        assert not sums[c.free].any()
        assert numpy.array_equal(bits(sums), bits(e.anchor_sums()))
        # rows of nodes without a term are exactly the unanchored values, and clearing the anchors
        # gives the unanchored buffer back
        e.set_anchors(None)
        assert not e.anchored and e.anchor_info() == (0, 0, 0) and not e.anchor_sums().any()
        e.grad()
        plain = e.read_exchange()
        assert numpy.array_equal(bits(plain[:3 * n].reshape(n, 3)[c.free]), bits(got[c.free]))
        assert not numpy.array_equal(plain, ex)
        e.set_coords(c.X)
        assert e.anchor_stress() == 0.0
    finally:
        e.close()
    # a solver that never had anchors gives that buffer too, bit for bit
    e = c.engine(0.0, q, anchors=False)
    try:
        e.set_bin_steps(c.scale)
        e.set_coords(c.X)
        e.grad()
        assert numpy.array_equal(bits(e.read_exchange()), bits(plain))
    finally:
        e.close()


@pytest.mark.parametrize("dtype", list(TOL))
def test_anchor_sums_are_exact_counts_for_q0_and_weight_1(dtype):
    n, count, _ = shapes(dtype)[3]
    c = case_of(dtype, n, count)
    e = c.engine(1.0, 0)
    try:
        want = (c.A > 0).sum(axis=0).astype(float)
        want[c.nodes] += (c.A > 0).sum(axis=1)
        assert numpy.array_equal(e.anchor_sums(), want)
        # the weight power set AFTER the anchors takes effect on them
        e.set_weight_power(2)
        s2 = am.sums_of(am.Terms(c.w, c.A, c.nodes, 1.0), 2)[1]
        assert numpy.abs(e.anchor_sums() - s2).max() <= 1e-12 * s2.max() and not numpy.array_equal(s2, want)
        e.set_coords(c.X)
        S2 = am.objective(c.X, am.Terms(c.w, c.A, c.nodes, 1.0), 2, dtype)[0]
        assert abs(e.stress() - S2) <= TOL[dtype] * S2
    finally:
        e.close()


def run_fit(c, lam, q, mu, iters=20):
    """The engine after `iters` anchored iterations with the model's steps, and those steps."""
    terms = am.Terms(c.w, c.A, c.nodes, lam)
    lr, factors = am.steps_of(am.sums_of(terms, q)[0])
    e = c.engine(lam, q)
    e.set_bin_steps(factors)
    e.set_momentum(mu)
    e.set_coords(c.X)
    e.iterate(iters, lr)
    return e, terms, lr, factors


def model_fit_with(c, terms, lr, factors, q, mu, iters):
    """am.fit with the step factors rounded to the run's dtype, as bb_solver_set_bin_steps holds them."""
    X, V = c.X.copy(), numpy.zeros_like(c.X)
    f = factors.astype(c.dtype).astype(numpy.float64)
    history = []
    for _ in range(iters):
        S, _, g = am.objective(X, terms, q, c.dtype)
        history.append(S)
        V = mu * V - lr * f[:, None] * g
        X = X + V
    return numpy.array(history), am.objective(X, terms, q, c.dtype)[1], X


FIT_CASES = [(d, i, q, mu) for d in TOL for i, q, mu in ((2, 0, 0.0), (3, 1, 0.5), (4, 2, 0.0))]


@pytest.mark.parametrize("dtype,which,q,mu", FIT_CASES)
def test_twenty_anchored_iterations_against_the_model(dtype, which, q, mu):
    n, count, _ = shapes(dtype)[which]
    c, lam, iters = case_of(dtype, n, count), 0.5, 20
    e, terms, lr, factors = run_fit(c, lam, q, mu, iters)
    try:
        history, Sa, X = model_fit_with(c, terms, lr, factors, q, mu, iters)
        got_h, got_X = e.stress_history(), e.get_coords()
        err_h = numpy.abs(got_h / history - 1).max()
        err_X = numpy.abs(got_X - X).max() / numpy.abs(X).max()
        print("%s n %d L' %d q %d mu %g: history %.2e, coordinates %.2e (relative)"
              % (dtype, n, count, q, mu, err_h, err_X))
        assert got_h.shape == (iters,) and err_h <= TOL[dtype] and err_X <= TOL[dtype]
        assert abs(e.anchor_stress() - Sa) <= TOL[dtype] * Sa
        assert e.iteration_path()[0] == "row_owner"   # a map of the one-launch path, which it left for these
        if mu == 0.0:
            # SPEC 2.4.1 carries over: non-increasing; fp32: but for one stress value's rounding
            slack = 0.0 if dtype == "float64" else n * 2.0 ** -24
            assert (numpy.diff(got_h) <= slack * got_h[:-1]).all() and got_h[-1] < got_h[0]
        # again: the same bits
        e2 = run_fit(c, lam, q, mu, iters)[0]
        try:
            assert numpy.array_equal(bits(e2.stress_history()), bits(got_h))
            assert numpy.array_equal(bits(e2.get_coords()), bits(got_X))
        finally:
            e2.close()
    finally:
        e.close()


@pytest.mark.parametrize("dtype", list(TOL))
def test_cleared_anchors_give_the_unanchored_continuation(dtype):
    n, count, _ = shapes(dtype)[2]
    c = case_of(dtype, n, count)
    e, _, lr, factors = run_fit(c, 0.5, 0, 0.0, 5)
    other = c.engine(2.0, 0)                        # another solver's anchors, alive all the while
    plain = c.engine(0.0, 0, anchors=False)
    try:
        X5 = e.get_coords()
        e.set_anchors(None)
        e.iterate(5, lr)
        plain.set_bin_steps(factors)
        plain.set_coords(X5)
        plain.iterate(5, lr)
        assert numpy.array_equal(bits(e.get_coords()), bits(plain.get_coords()))
        assert numpy.array_equal(bits(e.stress_history()[5:]), bits(plain.stress_history()))
        assert e.stress_history()[5] < e.stress_history()[4]          # (the landmark terms have left the sum)
    finally:
        for x in (e, other, plain):
            x.close()


def test_every_path_through_the_exchange_buffer_adds_the_terms():
    """bb_solver_iterate_dist's loop at world 1 and a group of one member go through bb_solver_grad's
    buffer; bb_solver_iterate_peer, which steps from the reduce itself, refuses."""
    from blueberry_amd.solver import GroupEngine
    dtype = "float64"
    n, count, _ = shapes(dtype)[2]
    c = case_of(dtype, n, count)
    e, _, lr, factors = run_fit(c, 0.5, 0, 0.0, 5)
    dev = bb.DeviceTriples(c.triples, 1, 0)
    g = GroupEngine(c.n, dtype, [0], tiles=dev.tiles(c.n, dtype))
    try:
        dev.per_device = {0: dev}
        g.set_wish_triples(dev, "wish", 3.0)
        with dev.shortest_paths(c.n, c.sources, kind="wish") as rows:
            g.members[0].set_anchors(rows, c.kept, 0.5)
        g.set_bin_steps(factors)
        g.set_coords(c.X)
        g.iterate(5, lr)
        g.sync()
        assert numpy.abs(g.stress_history() / e.stress_history() - 1).max() <= TOL[dtype]
        assert numpy.abs(g.get_coords() - e.get_coords()).max() <= TOL[dtype] * numpy.abs(c.X).max()
        with pytest.raises(RuntimeError, match="landmark anchors"):
            e.iterate_peer(1, lr)
        # grad / apply by hand: the same bits as the iterate loop
        again = run_fit(c, 0.5, 0, 0.0, 0)[0]
        for _ in range(5):
            again.grad()
            again.apply(lr)
        assert numpy.array_equal(bits(again.get_coords()), bits(e.get_coords()))
        assert numpy.array_equal(bits(again.stress_history()), bits(e.stress_history()))
        again.close()
    finally:
        g.close()
        e.close()
        dev.close()


def _set_anchors_status(eng, rows_handle, kept, weight):
    k = None if kept is None else numpy.ascontiguousarray(kept, dtype=numpy.uint8)
    rc = _lib.load().bb_solver_set_anchors(eng._h, rows_handle,
                                           None if k is None else k.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                           float(weight))
    return rc, _lib.last_error()


def test_set_anchors_refusals_and_handle_lifetimes():
    dtype = "float64"
    vw = VW[dtype]
    c = case_of(dtype, vw + 1, 65)
    dev = bb.DeviceTriples(c.triples, 1, 0)
    rows = dev.shortest_paths(c.n, c.sources, kind="wish")
    e = c.engine(0.0, 0, anchors=False)
    try:
        for weight, word in ((-1.0, "weight"), (float("nan"), "weight"), (float("inf"), "weight")):
            rc, msg = _set_anchors_status(e, rows._h, c.kept, weight)
            assert rc == _lib.BB_ERR_INVALID and word in msg
        rc, msg = _set_anchors_status(e, rows._h, numpy.zeros(c.sources.size), 1.0)
        assert rc == _lib.BB_ERR_INVALID and "fewer than 1 kept row" in msg
        dup = dev.shortest_paths(c.n, [5, 9, 5], kind="wish")
        rc, msg = _set_anchors_status(e, dup._h, None, 1.0)
        assert rc == _lib.BB_ERR_INVALID and "same source node" in msg
        dup.close()
        other = HipEngine(c.n + 3, dtype)
        rc, msg = _set_anchors_status(other, rows._h, c.kept, 1.0)
        assert rc == _lib.BB_ERR_INVALID and "n_nodes != n_bins" in msg
        other.close()
        ranked = HipEngine(c.n, dtype, rank=0, world=2)
        rc, msg = _set_anchors_status(ranked, rows._h, c.kept, 1.0)
        assert rc == _lib.BB_ERR_STATE and "world > 1" in msg
        ranked.close()
        many = HipEngine(2 * vw, dtype, tiles=([0, 1], [0, 1]))
        many.set_maps([0, vw, 2 * vw], [1.0, 1.0])
        two = bb.DeviceTriples(numpy.array([[0.0, 1.0, 1.0], [1.0, 2.0, 1.0]]), 1, 0)
        with two.shortest_paths(2 * vw, [0], kind="wish") as r2:
            rc, msg = _set_anchors_status(many, r2._h, None, 1.0)
            assert rc == _lib.BB_ERR_STATE and "several maps" in msg
        two.close()
        many.close()
        # after every refusal the solver is as it was, and usable
        assert not e.anchored and e.anchor_info() == (0, 0, 0)
        e.set_anchors(rows, c.kept, 0.5)
        assert e.anchored
        with pytest.raises(RuntimeError, match="landmark anchors"):
            e.set_maps([0, c.n], [1.0])
        e.set_coords(c.X)
        e.grad()
        with pytest.raises(RuntimeError, match="bb_solver_grad is pending"):
            e.set_anchors(None)
        e.apply(1e-4)
        # a refused replacement keeps the anchors that are there
        before = e.anchor_info()
        with pytest.raises(ValueError, match="weight"):
            e.set_anchors(rows, c.kept, -2.0)
        assert e.anchor_info() == before
        # the paths go first, then the triples; the engine goes on; closed rows are a ValueError
        S = e.stress()
        rows.close()
        dev.close()
        assert e.stress() == S
        e.iterate(2, 1e-4)
        with pytest.raises(ValueError, match="closed"):
            e.set_anchors(rows, c.kept, 0.5)
        assert e.anchor_info() == before
        # the engine goes before paths that are still open
        dev2 = bb.DeviceTriples(c.triples, 1, 0)
        rows2 = dev2.shortest_paths(c.n, c.sources, kind="wish")
        e2 = c.engine(0.0, 0, anchors=False)
        e2.set_anchors(rows2, c.kept, 0.5)
        e2.close()
        assert rows2.reached().shape == (c.sources.size,)
        rows2.close()
        rows2.close()
        dev2.close()
    finally:
        e.close()
        rows.close()
        dev.close()


# ---- the Python route ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chain():
    """tests/test_gpu_landmark.py's map with a second component (a dropped landmark, bins that are
    not placed), as 'counts' triples over 460 nodes."""
    triples = am.hic_like_triples(400, 1)[0]
    i = numpy.arange(410.0, 449.0)
    return numpy.concatenate([triples, numpy.stack([i, i + 1, numpy.full(i.size, 5.0)], axis=1)]), 459


def _same_fit(a, b):
    return numpy.array_equal(bits(a.structure_), bits(b.structure_)) and numpy.array_equal(bits(a.stress_), bits(b.stress_))


@pytest.mark.parametrize("dtype", list(TOL))
def test_weight_zero_is_the_landmark_fit_bit_for_bit(chain, dtype):
    import scipy.sparse
    t, n_bins = chain
    kw = dict(n_iter=6, dtype=dtype, degree_steps=True, seed=2)
    today = bb.StructureSolver(init=("landmark", 16), **kw).fit_triples(t, 1, n_bins)
    zero = bb.StructureSolver(init=("landmark", 16, 0.0), **kw).fit_triples(t, 1, n_bins)
    assert _same_fit(today, zero) and zero.landmark_terms_ == 0 and zero.anchor_stress_ == 0.0
    assert _same_fit(bb.StructureSolver(init=("landmark", 16, 0.0), **dict(kw, degree_steps=False)).fit_triples(t, 1, n_bins),
                     bb.StructureSolver(init=("landmark", 16), **dict(kw, degree_steps=False)).fit_triples(t, 1, n_bins))
    C = numpy.zeros((n_bins + 1, n_bins + 1))
    C[t[:, 0].astype(int), t[:, 1].astype(int)] = t[:, 2]
    sp = scipy.sparse.coo_matrix(C)
    assert _same_fit(bb.StructureSolver(init=("landmark", 16), **kw).fit(sp),
                     bb.StructureSolver(init=("landmark", 16, 0.0), **kw).fit(sp))
    # with a weight: another fit, the same from both routes, the same bits twice
    a = bb.StructureSolver(init=("landmark", 16, 0.5), **kw).fit_triples(t, 1, n_bins)
    assert not _same_fit(a, today) and a.landmark_terms_ > 0 and a.anchor_stress_ > 0
    assert numpy.array_equal(a.landmarks_, today.landmarks_)
    assert numpy.array_equal(a.landmark_placed_, today.landmark_placed_)
    assert _same_fit(a, bb.StructureSolver(init=("landmark", 16, 0.5), **kw).fit_triples(t, 1, n_bins))
    assert _same_fit(a, bb.StructureSolver(init=("landmark", 16, 0.5), **kw).fit(sp))


@pytest.mark.parametrize("dtype,q,mu", [("float64", 0, 0.0), ("float32", 2, 0.0), ("float64", 1, 0.5)])
def test_fit_triples_with_landmark_weight_against_the_model(chain, dtype, q, mu):
    t, n_bins = chain
    n, lam, iters = n_bins + 1, 0.25, 20
    start, info = bb.landmark_start(t, 1, n_bins, n_landmarks=16, seed=2, return_info=True)
    assert not info.kept_.all() and not info.placed_.all()
    w64 = lm.weights_of(t, 1, n, kind="counts", alpha=3.0)
    w = im.matrix_of("triples", n, dtype, kind="counts", alpha=3.0, triples=t, resolution=1)
    A, nodes = am.anchors_of(lm.geodesics(w64, info.landmarks_), info.landmarks_, info.kept_, dtype)
    terms = am.Terms(w, A, nodes, lam)
    s = am.sums_of(terms, q)[0]
    lr, factors = am.steps_of(s)
    X0 = start.astype(dtype).astype(numpy.float64)
    fit = bb.StructureSolver(n_iter=iters, dtype=dtype, degree_steps=True, weight_power=q, momentum=mu, seed=2,
                             init=("landmark", 16, lam)).fit_triples(t, 1, n_bins)
    # an array given to the call replaces the start only: the constraints stay
    again = bb.StructureSolver(n_iter=iters, dtype=dtype, degree_steps=True, weight_power=q, momentum=mu, seed=5,
                               init=("landmark", 16, lam)).fit_triples(t, 1, n_bins, init=start)
    assert _same_fit(fit, again)

    class Run(object):
        pass
    c = Run()
    c.X, c.dtype = X0, dtype
    history, Sa, X = model_fit_with(c, terms, lr, factors, q, mu, iters)
    n_terms = (A > 0).sum() + n
    assert abs(fit.lr_ - lr) <= n_terms * 2.0 ** -52 * lr + 1e-12 * lr        # (counts: the device's pow, SPEC 4)
    err_h = numpy.abs(fit.stress_ / history - 1).max()
    err_X = numpy.abs(fit.structure_ - X).max() / numpy.abs(X).max()
    print("%s q %d mu %g: history %.2e, coordinates %.2e, anchor stress %.6g (model %.6g)"
          % (dtype, q, mu, err_h, err_X, fit.anchor_stress_, Sa))
    assert fit.stress_.shape == (iters,) and err_h <= TOL[dtype] and err_X <= TOL[dtype]
    assert abs(fit.anchor_stress_ - Sa) <= TOL[dtype] * Sa
    assert fit.landmark_terms_ == int((A > 0).sum())
    if mu == 0.0:
        slack = 0.0 if dtype == "float64" else n * 2.0 ** -24
        assert (numpy.diff(fit.stress_) <= slack * fit.stress_[:-1]).all()


def test_python_refusals_on_the_device(chain):
    t, n_bins = chain
    s = bb.StructureSolver(init=("landmark", 16, 0.5), degree_steps=True, n_iter=1)
    with pytest.raises(ValueError, match="init='landmark' with landmark_weight > 0 keeps its constraints on one device"):
        s._check_anchor_devices(2)                      # a torch.distributed world of 2
    with pytest.raises(ValueError, match="init='landmark' does not go with complete='shortest_path'"):
        s.fit_triples(t, 1, n_bins, complete="shortest_path")
    with pytest.raises(ValueError, match="init='landmark' needs a sparse input"):
        s.fit(numpy.ones((8, 8)))
    with pytest.raises(ValueError, match="init='landmark' is not for fit_many"):
        s.fit_many([numpy.ones((8, 8))])
    # a refused fit leaves no rows behind, and the solver fits afterwards
    with pytest.raises(ValueError, match="too disconnected"):
        s.fit_triples(numpy.array([[0.0, 1.0, 3.0]]), 1, 20)
    assert s._anchor is None
    assert s.fit_triples(t, 1, n_bins).landmark_terms_ > 0 and s._anchor is None


def test_the_constraints_hold_the_global_fold():
    """hic_like_triples(1000, 1), 32 landmarks, float64, q = 0, degree_steps, 1000 iterations.  The
    model (tests/test_anchor_model_cpu.py) gives Spearman 0.870 at the start, 0.840 with
    landmark_weight = 0.1 and 0.663 without: margins of 0.03 and 0.18 over the thresholds."""
    n = 1000
    triples, Ds, _, _ = am.hic_like_triples(n, 1)
    kw = dict(n_iter=1000, dtype="float64", kind="counts", alpha=3.0, degree_steps=True)
    start = bb.landmark_start(triples, 1, n - 1, n_landmarks=32)
    anchored = bb.StructureSolver(init=("landmark", 32, 0.1), **kw).fit_triples(triples, 1, n - 1)
    plain = bb.StructureSolver(init=("landmark", 32, 0.0), **kw).fit_triples(triples, 1, n - 1)
    r_start, r_anchored, r_plain = (am.spearman(X, Ds) for X in (start, anchored.structure_, plain.structure_))
    print("Spearman: landmark start %.3f, 1000 iterations with landmark_weight 0.1 %.3f, without %.3f; stress "
          "%.0f -> %.0f (of which landmark terms %.0f) and %.0f -> %.0f"
          % (r_start, r_anchored, r_plain, anchored.stress_[0], anchored.stress_[-1], anchored.anchor_stress_,
             plain.stress_[0], plain.stress_[-1]))
    assert r_anchored >= r_start - 0.06
    assert r_anchored - r_plain >= 0.08
    assert (numpy.diff(anchored.stress_) <= 0).all()
