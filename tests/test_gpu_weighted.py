"""GPU: the weighted stress of docs/SPEC.md 2.3.1 (S_q = sum delta^-q (d - delta)^2, q = 1 Sammon,
q = 2 relative stress) on every kernel instantiation, size edge and solver path that carries it,
against the weighted C oracle (oracle/bb_oracle.c bbo_stress_grad_units_weighted, oracle/
bb_oracle_mt.c bbo_solve_gen_weighted_mt; pinned to the numpy model of test_weighted_stress.py in
test_oracle.py).  Tolerances as for q = 0: fp64 1e-12, fp32 1e-5, relative, on every entry of the
stress history and on the max-abs coordinates."""
import functools

import numpy
import pytest

import blueberry_amd as bb
from blueberry_amd.solver import HipEngine, layout_info, weighted_steps
from tests import _oracle
from tests._util import host_threads as _host_threads
from tests._util import rel as _rel
from tests._util import solver_path as path         # noqa: F401 -- the fixture, under this file's name
from tests.test_weighted_stress import count_map, start, weights, wish_of

pytestmark = pytest.mark.gpu

TOL = {"float64": 1e-12, "float32": 1e-5}
NT_BYTES = 240 << 20          # build_indices: non-temporal loads once a rank's units exceed this
UNIT_BYTES = 8192


def _close(X, h, X_ref, h_ref, dtype):
    tol = TOL[dtype]
    assert h.shape == h_ref.shape
    err_s, err_x = float(numpy.abs(h / h_ref - 1).max()), float(_rel(X, X_ref))
    assert err_s < tol and err_x < tol, (dtype, err_s, err_x)
    return err_s, err_x


def _counts(n, seed):
    """A Hi-C-like count map with dead bins, missing pairs and NaN / inf entries; for the
    smallest sizes a complete map with one missing pair."""
    if n >= 16:
        return count_map(n, seed=seed)
    rng = numpy.random.default_rng(seed)
    i, j = numpy.indices((n, n))
    c = numpy.triu(rng.poisson(200.0 * numpy.maximum(numpy.abs(i - j), 1) ** -1.08) + 1.0, 1)
    if n >= 7:
        c[1, n - 2] = 0.0
    return c + c.T


@functools.lru_cache(maxsize=None)
def _problem(n, dtype, seed=0):
    W = wish_of(_counts(n, seed + n), dtype)
    return W, start(n, W)


def _lr(W, q):
    return 1.0 / (2.0 * weights(W, q).sum(1).max())


@functools.lru_cache(maxsize=None)
def _reference(n, dtype, q, k, mu=0.0, scaled=False):
    """The oracle's K steps on _problem(n, dtype) (cached: every path and variant compares with it)."""
    W, x0 = _problem(n, dtype)
    s = weights(W, q).sum(1)
    scale = numpy.where(s > 0, s.max() / numpy.where(s > 0, s, 1.0), 1.0) if scaled else None
    X, h = _oracle.load().solve_weighted(W, x0, k, _lr(W, q), q, mu=mu, bin_scale=scale,
                                         f64=dtype == "float64")
    return X, h, scale


def _engine(n, dtype, W, q, tiles=None):
    eng = HipEngine(n, dtype, tiles=tiles)
    eng.set_wish_dense(W, "wish", 3.0)
    eng.set_weight_power(q)
    return eng


def _run(n, dtype, W, q, x0, k, lr, mu=0.0, scale=None):
    eng = _engine(n, dtype, W, q)
    try:
        if mu:
            eng.set_momentum(mu)
        if scale is not None:
            eng.set_bin_steps(scale)
        eng.set_coords(x0)
        eng.iterate(k, lr)
        return eng.get_coords(), eng.stress_history(), eng.iteration_path()
    finally:
        eng.close()


def _want_path(n, path):
    """What iteration_path() must report: ('row_owner', WPR) or ('units', 0)."""
    if path == "row_owner" and n <= 4096:
        return ("row_owner", 4 if n <= 1024 else (2 if n <= 2048 else 1))
    return ("units", 0)


# ---- ragged sizes: every row-owner WPR with Q = 1, 2, and the 4,096 / 4,097 switch ------------
@pytest.mark.parametrize("q", [1, 2])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("n", [2, 3, 7, 8, 9, 127, 128, 129, 255, 256, 257, 513, 1024, 1025,
                               2048, 2049, 4096, 4097])
def test_weighted_ragged_sizes(n, dtype, q, path):
    k = 5
    W, x0 = _problem(n, dtype)
    X_ref, h_ref, _ = _reference(n, dtype, q, k)
    X, h, got = _run(n, dtype, W, q, x0, k, _lr(W, q))
    assert got == _want_path(n, path)
    _close(X, h, X_ref, h_ref, dtype)


# ---- the unit sweep: layout x WPB x reduce / descriptor variants, then NT by size ----------------
_LAYOUTS = {"fp32": ("float32", 5000, 10), "fp64_narrow": ("float64", 3000, 3),
            "fp64_wide": ("float64", 4300, 3)}
_VARIANTS = {"default": {}, "wpb8": {"BB_WAVES_PER_CU": "8"},
             "wpb4_unpaired": {"BB_WAVES_PER_CU": "4", "BB_PAIR": "0"},
             "reduce4": {"BB_REDUCE_SLICES": "4"}, "reduce8": {"BB_REDUCE_SLICES": "8"},
             "table_desc": {"BB_ARITH_DESC": "0"}}


@pytest.mark.parametrize("q", [1, 2])
@pytest.mark.parametrize("variant", sorted(_VARIANTS))
@pytest.mark.parametrize("layout", sorted(_LAYOUTS))
def test_weighted_sweep_variants(layout, variant, q, monkeypatch):
    """Count maps with holes, dead bins and NaN / inf entries, on the unit sweep of each layout
    (fp32, fp64 narrow 128 x 8 units, fp64 wide 512 x 2) with each run-time variant."""
    dtype, n, k = _LAYOUTS[layout]
    monkeypatch.setenv("BB_ROW_OWNER_MAX", "0")
    for key, v in _VARIANTS[variant].items():
        monkeypatch.setenv(key, v)
    lay = layout_info(n, dtype)
    assert lay["vw"] == (128 if layout == "fp64_narrow" else 512)
    assert lay["n_units"] * UNIT_BYTES <= NT_BYTES           # NT is covered by size below
    W, x0 = _problem(n, dtype)
    assert (W == 0).all(axis=1).any()                         # a dead bin
    X_ref, h_ref, _ = _reference(n, dtype, q, k)
    X, h, got = _run(n, dtype, W, q, x0, k, _lr(W, q))
    assert got == ("units", 0)
    _close(X, h, X_ref, h_ref, dtype)


def _generated(n, dtype, q, k, lr=None, mu=0.0, bin_scale=None, tiles=None):
    """The oracle's run on delta_ij = |x*_i - x*_j| formed pair by pair (rounded to float as
    the device stores it in fp32)."""
    xs = _oracle.random_walk(n)
    x0 = _oracle.noisy_init(xs)
    X, h = _oracle.solve_gen_mt(xs, x0, k, lr, _host_threads(), tiles=tiles, mu=mu,
                                f64=dtype == "float64", bin_scale=bin_scale, q=q)
    return xs, x0, X, h


def _auto_lr_generated(n, dtype, q, xs):
    """lr = 1 / (2 max s) from the device's weighted degrees of the generated map."""
    eng = HipEngine(n, dtype)
    try:
        eng.set_wish_from_coords(xs)
        eng.set_weight_power(q)
        return weighted_steps(eng.weight_sums(), n, dtype, "auto", False)[0]
    finally:
        eng.close()


@pytest.mark.parametrize("q", [1, 2])
@pytest.mark.parametrize("wpb", [4, 8])
@pytest.mark.parametrize("dtype,n,k", [("float32", 12000, 5), ("float64", 8500, 3)])
def test_weighted_sweep_nontemporal(dtype, n, k, wpb, q, monkeypatch):
    """The non-temporal sweep (a rank's units exceed 240 MiB: no environment switch reaches
    it, so the size does), with 4 and 8 waves per workgroup."""
    lay = layout_info(n, dtype)
    assert lay["vw"] == 512 and lay["n_units"] * UNIT_BYTES > NT_BYTES
    assert lay["n_units"] < 65000                             # 4 waves per CU unless set
    if wpb == 8:
        monkeypatch.setenv("BB_WAVES_PER_CU", "8")
    xs = _oracle.random_walk(n)
    lr = _auto_lr_generated(n, dtype, q, xs)
    _, x0, X_ref, h_ref = _generated(n, dtype, q, k, lr)
    eng = HipEngine(n, dtype)
    try:
        eng.set_wish_from_coords(xs)
        eng.set_weight_power(q)
        eng.set_coords(x0)
        eng.iterate(k, lr)
        assert eng.iteration_path() == ("units", 0)
        _close(eng.get_coords(), eng.stress_history(), X_ref, h_ref, dtype)
    finally:
        eng.close()


# ---- full size ---------------------------------------------------------------------------------
@pytest.mark.parametrize("q", [1, 2])
@pytest.mark.parametrize("dtype,k", [("float32", 20), ("float64", 6)])
def test_weighted_full_size_chr1_10kb(dtype, k, q):
    """N = 24,926 (chr1 at 10 kb): NT loads and 8 waves per workgroup by default."""
    n = 24926
    lay = layout_info(n, dtype)
    assert lay["n_units"] * UNIT_BYTES > NT_BYTES and lay["n_units"] >= 65000
    xs = _oracle.random_walk(n)
    lr = _auto_lr_generated(n, dtype, q, xs)
    _, x0, X_ref, h_ref = _generated(n, dtype, q, k, lr)
    eng = HipEngine(n, dtype)
    try:
        eng.set_wish_from_coords(xs)
        eng.set_weight_power(q)
        eng.set_coords(x0)
        eng.iterate(k, lr)
        err = _close(eng.get_coords(), eng.stress_history(), X_ref, h_ref, dtype)
    finally:
        eng.close()
    print("weighted N=%d K=%d q=%d %s vs oracle: stress %.2e coords %.2e" % ((n, k, q, dtype) + err))


def test_weighted_genome10kb_with_bin_steps():
    """The README's weighted workload: the N = 309,568 blocked-sparse genome map in fp32, q = 2,
    K = 3 with lr = 1 / (2 max s) and the per-bin steps max s / s_i (weight_sums ->
    weighted_steps -> set_bin_steps).  A sample of s_i is checked on the host."""
    from blueberry_amd.solver import tiles_from_blocks
    from blueberry_amd.utils import genome_boundaries
    n, k, q, vw = 309568, 3, 2, 512
    tiles, pairs = tiles_from_blocks(n, genome_boundaries(n), 1000, "float32")
    assert pairs == 2544233312
    xs = _oracle.random_walk(n)
    x0 = _oracle.noisy_init(xs)
    eng = HipEngine(n, "float32", tiles=tiles)
    try:
        eng.set_wish_from_coords(xs)
        eng.set_weight_power(q)
        s = eng.weight_sums()
        # s_i on the host for a few bins: every partner j in a stored tile, delta rounded to float
        nb = -(-n // vw)
        have = numpy.zeros((nb, nb), dtype=bool)
        have[tiles[0], tiles[1]] = True
        have |= have.T
        for i in numpy.random.default_rng(0).choice(n, 12, replace=False):
            j = numpy.concatenate([numpy.arange(b * vw, min(n, (b + 1) * vw))
                                   for b in numpy.flatnonzero(have[i // vw])])
            j = j[j != i]
            d = numpy.sqrt(((xs[j] - xs[i]) ** 2).sum(1)).astype(numpy.float32).astype(numpy.float64)
            want = (1.0 / (d[d > 0] ** 2)).sum()
            assert abs(s[i] / want - 1) < 1e-12, (i, s[i], want)
        lr, scale = weighted_steps(s, n, "float32", "auto", True)
        assert scale is not None and scale.max() > 2.0
        eng.set_bin_steps(scale)
        eng.set_coords(x0)
        eng.iterate(k, lr)
        X, h = eng.get_coords(), eng.stress_history()
    finally:
        eng.close()
    X_ref, h_ref = _oracle.solve_gen_mt(xs, x0, k, lr, _host_threads(), tiles=tiles, f64=False,
                                        bin_scale=scale, q=q)
    err = _close(X, h, X_ref, h_ref, "float32")
    assert (numpy.diff(h) < 0).all()
    print("weighted genome10kb N=%d K=%d q=2 fp32 with per-bin steps: stress %.2e coords %.2e"
          % ((n, k) + err))


# ---- solver paths --------------------------------------------------------------------------------
@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("mu", [0.3, 0.6])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_weighted_momentum_and_bin_steps(dtype, mu, scaled, path):
    n, k, q = 1500, 12, 2
    W, x0 = _problem(n, dtype)
    X_ref, h_ref, scale = _reference(n, dtype, q, k, mu, scaled)
    X, h, got = _run(n, dtype, W, q, x0, k, _lr(W, q), mu=mu, scale=scale)
    assert got == _want_path(n, path)
    _close(X, h, X_ref, h_ref, dtype)


@pytest.mark.parametrize("q", [1, 2])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_weighted_engine_stress_is_s_q(dtype, q, path):
    n = 1100
    W, x0 = _problem(n, dtype)
    s_ref, _ = _oracle.load().stress_grad_weighted(W, x0, q, f64=dtype == "float64")
    eng = _engine(n, dtype, W, q)
    try:
        eng.set_coords(x0)
        assert abs(eng.stress() / s_ref - 1) < TOL[dtype]
        assert eng.iteration_path() == _want_path(n, path)
    finally:
        eng.close()


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_weighted_split_iterate_calls_are_bit_identical(dtype, path):
    """1 + 2 + 4 iterations over three calls equal 7 in one (the row-owner fold between calls)."""
    n, q = 1300, 2
    W, x0 = _problem(n, dtype)
    lr = _lr(W, q)
    out = []
    for calls in ((7,), (1, 2, 4)):
        eng = _engine(n, dtype, W, q)
        try:
            eng.set_coords(x0)
            for c in calls:
                eng.iterate(c, lr)
            out.append((eng.get_coords(), eng.stress_history()))
            assert eng.iteration_path() == _want_path(n, path)
        finally:
            eng.close()
    assert numpy.array_equal(out[0][0], out[1][0]) and numpy.array_equal(out[0][1], out[1][1])


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_weighted_power_change_mid_run_keeps_the_history(dtype, path):
    """q = 0 for k1 steps, then q = 2 for k2: the history is the two runs' histories end to end."""
    n, k1, k2 = 900, 4, 5
    W, x0 = _problem(n, dtype)
    o = _oracle.load()
    f64 = dtype == "float64"
    lr0, lr2 = _lr(W, 0), _lr(W, 2)
    X1, h1 = o.solve_weighted(W, x0, k1, lr0, 0, f64=f64)
    X2, h2 = o.solve_weighted(W, X1, k2, lr2, 2, f64=f64)
    eng = _engine(n, dtype, W, 0)
    try:
        eng.set_coords(x0)
        eng.iterate(k1, lr0)
        eng.set_weight_power(2)
        eng.iterate(k2, lr2)
        _close(eng.get_coords(), eng.stress_history(), X2, numpy.concatenate([h1, h2]), dtype)
    finally:
        eng.close()


@pytest.mark.parametrize("n", [963, 5000])
def test_weighted_tol_stops_at_the_models_iteration(n):
    """fit(tol=..., weight_power=2): the check every `check_every` steps compares S_q; tol is put
    between the model's relative decreases at the checks so that each decision has a margin."""
    dtype, q, every, top = "float64", 2, 5, 60
    C = _counts(n, 40)
    W = wish_of(C, dtype)
    x0 = start(n, W)
    _, h = _oracle.load().solve_weighted(W, x0, top, _lr(W, q), q)
    checks = numpy.arange(every, top + 1, every)
    rel = numpy.abs(h[checks - 2] - h[checks - 1]) / h[checks - 2]
    stop = 3                                            # stop at the 4th check
    assert rel[stop] < rel[:stop].min()
    tol = float(numpy.sqrt(rel[stop] * rel[:stop].min()))
    margins = numpy.abs(rel[:stop + 1] - tol) / tol
    assert margins.min() > 1e-6, margins
    sol = bb.StructureSolver(n_iter=top, dtype=dtype, weight_power=q, tol=tol,
                             check_every=every).fit(C, init=x0)
    assert sol.n_iter_ == checks[stop]
    assert numpy.abs(sol.stress_ / h[:checks[stop]] - 1).max() < 1e-12


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_weighted_spectral_start_is_unweighted(dtype, path):
    """The spectral start uses the (D o D) matvec: a weight power set on the solver changes no
    bit of it."""
    n = 1200
    W, _ = _problem(n, dtype)
    v0 = numpy.random.default_rng(2).standard_normal((n, 3))
    out = []
    for q in (0, 2):
        eng = _engine(n, dtype, W, q)
        try:
            eng.spectral_init_device(40, v0, tol=1e-3)
            out.append(eng.get_coords())
            assert eng.iteration_path() == _want_path(n, path)
        finally:
            eng.close()
    assert numpy.array_equal(out[0], out[1])


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_weighted_sparse_and_triples_input(dtype):
    """scipy.sparse and fit_triples input with weight_power=2 and lr='auto' against the oracle."""
    import scipy.sparse
    n, k, q, res = 1400, 8, 2, 10000
    C = _counts(n, 9)
    C[~numpy.isfinite(C)] = 0.0
    W = wish_of(C, dtype)
    x0 = start(n, W)
    lr = _lr(W, q)
    X_ref, h_ref = _oracle.load().solve_weighted(W, x0, k, lr, q, f64=dtype == "float64")
    sol = bb.StructureSolver(n_iter=k, dtype=dtype, weight_power=q).fit(
        scipy.sparse.coo_matrix(numpy.triu(C, 1)), init=x0)
    assert abs(sol.lr_ / lr - 1) < 1e-14
    _close(sol.structure_, sol.stress_, X_ref, h_ref, dtype)
    bi, bj = numpy.nonzero(numpy.triu(C, 1))
    triples = numpy.stack([bi * float(res), bj * float(res), C[bi, bj]], 1)
    tri = bb.StructureSolver(n_iter=k, dtype=dtype, weight_power=q).fit_triples(
        triples, res, n - 1, init=x0)
    assert abs(tri.lr_ / lr - 1) < 1e-14
    _close(tri.structure_, tri.stress_, X_ref, h_ref, dtype)


# ---- numeric edges ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [300, 1500])
def test_weighted_float32_q1_smallest_accepted_wish_distance(n, monkeypatch):
    """fp32, q = 1: a pair at delta = 2^-60 (s_i = 2^60, the largest accepted) gives finite
    results on both paths; 2^-61 is refused before iterating (the q = 2 twin is in
    test_weighted_stress.py)."""
    if n > 1000:
        monkeypatch.setenv("BB_ROW_OWNER_MAX", "0")
    rng = numpy.random.default_rng(6)
    W = numpy.triu(1.0 + rng.random((n, n)), 1)
    W = W + W.T
    W2 = W.copy()
    W[3, 4] = W[4, 3] = numpy.float32(2.0 ** -60)
    W2[3, 4] = W2[4, 3] = numpy.float32(2.0 ** -61)
    for M in (W, W2):                                   # bins 3 and 4 keep only that pair
        for b in (3, 4):
            keep = M[b, 7 - b]
            M[b, :] = 0.0
            M[:, b] = 0.0
            M[b, 7 - b] = M[7 - b, b] = keep
    x0 = rng.standard_normal((n, 3))
    s = bb.StructureSolver(n_iter=10, dtype="float32", kind="wish", weight_power=1).fit(W, init=x0)
    assert numpy.all(numpy.isfinite(s.structure_)) and numpy.all(numpy.isfinite(s.stress_))
    assert s.lr_ == 1.0 / (2.0 * 2.0 ** 60)
    with pytest.raises(ValueError):
        bb.StructureSolver(n_iter=10, dtype="float32", kind="wish", weight_power=1).fit(W2, init=x0)


@pytest.mark.parametrize("q", [1, 2])
@pytest.mark.parametrize("dtype,e", [("float64", 300), ("float64", -300), ("float32", 20),
                                     ("float32", -20)])
def test_weighted_scale_equivariance(dtype, e, q, path):
    """Scaling delta and X_0 by c = 2^e scales X_k by c and S_q by c^(2 - q) with lr='auto':
    the weights and reciprocals far from delta ~ 1 (fp64 rcp_f64, fp32 v_rcp_f32)."""
    n, k = 700, 8
    W, x0 = _problem(n, dtype)
    c = 2.0 ** e
    runs = []
    for f in (1.0, c):
        sol = bb.StructureSolver(n_iter=k, dtype=dtype, kind="wish", weight_power=q).fit(
            W * f, init=x0 * f)
        assert numpy.all(numpy.isfinite(sol.structure_)) and numpy.all(sol.stress_ > 0)
        runs.append(sol)
    a, b = runs
    assert abs(b.lr_ / (a.lr_ * c ** q) - 1) < 1e-14
    _close(b.structure_ / c, b.stress_ / c ** (2 - q), a.structure_, a.stress_, dtype)
    eng = _engine(n, dtype, W * c, q)
    try:
        assert eng.iteration_path() == _want_path(n, path)
    finally:
        eng.close()
