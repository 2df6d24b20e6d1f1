"""Weighted stress (docs/SPEC.md 2.3.1): S_q = sum w (d - delta)^2 with w = delta^-q, q = 1
(Sammon) and q = 2 (relative stress), against a numpy float64 model of SPEC 2.3.1 / 2.4 /
2.4.1 that lives in this file.  tests/test_oracle.py pins the weighted C oracle to this model, and
tests/test_gpu_weighted.py holds the kernels against that oracle at every size and variant."""
import numpy
import pytest

import blueberry_amd as bb
from blueberry_amd.solver import HipEngine, tiles_from_blocks, weighted_steps
from tests._util import rel as _rel


# --------------------------------------------------------------------------
# numpy float64 model
# --------------------------------------------------------------------------
def weights(W, q):
    """w_ij = delta_ij^-q where delta > 0, else exactly 0 (never inf * 0)."""
    mask = W > 0
    return numpy.where(mask, numpy.where(mask, W, 1.0) ** (-float(q)), 0.0)


def stress_grad(W, X, q, eps2=1e-300, block=512):
    """(S_q(X), g(X)) of SPEC 2.3.1, both triangles of the symmetric W, in row blocks."""
    n = W.shape[0]
    S, g = 0.0, numpy.zeros_like(X)
    for a in range(0, n, block):
        b = min(n, a + block)
        D = X[a:b, None, :] - X[None, :, :]
        d = numpy.sqrt((D * D).sum(-1) + eps2)
        w = W[a:b]
        mask = w > 0
        res = numpy.where(mask, d - w, 0.0)
        wq = weights(w, q)
        S += 0.5 * (wq * res * res).sum()
        g[a:b] = 2.0 * ((wq * res / d)[:, :, None] * D).sum(1)
    return S, g


def model(W, X0, K, lr, q, scale=None):
    """K steps X <- X - lr * scale * g; returns (X_K, [S_q(X_0) .. S_q(X_{K-1})])."""
    X, hist = X0.copy(), []
    for _ in range(K):
        S, g = stress_grad(W, X, q)
        hist.append(S)
        if scale is not None:
            g = g * scale[:, None]
        X = X - lr * g
    return X, numpy.array(hist)


def count_map(n, seed=0, dead=None, bad=3):
    """An incomplete Hi-C-like count map: counts ~ Poisson(200 |i-j|^-1.08), pairs thinned
    with distance, dead bins, and a few NaN / inf entries (no constraint, SPEC 2.1)."""
    rng = numpy.random.default_rng(seed)
    i, j = numpy.meshgrid(numpy.arange(n), numpy.arange(n), indexing="ij")
    sep = numpy.abs(i - j)
    c = rng.poisson(200.0 * numpy.maximum(sep, 1) ** -1.08).astype(float)
    c *= rng.random((n, n)) < numpy.exp(-sep / (0.3 * n))
    c = numpy.triu(c, 1)
    dead = rng.choice(n, max(1, n // 40), replace=False) if dead is None else dead
    c[dead, :] = 0.0
    c[:, dead] = 0.0
    for k in range(bad):
        a = int(rng.integers(0, n - 2))
        c[a, a + 1 + k] = numpy.nan if k % 2 == 0 else numpy.inf
    return c + c.T


def wish_of(C, dtype, alpha=3.0):
    """delta = c^(-1/alpha) for finite c > 0, else 0, rounded to the solver's dtype."""
    ok = numpy.isfinite(C) & (C > 0)
    W = numpy.where(ok, numpy.where(ok, C, 1.0) ** (-1.0 / alpha), 0.0)
    numpy.fill_diagonal(W, 0.0)
    return W.astype(dtype).astype(numpy.float64)


def start(n, W, seed=1):
    return numpy.random.default_rng(seed).standard_normal((n, 3)) * float(numpy.median(W[W > 0]))


# --------------------------------------------------------------------------
# CPU
# --------------------------------------------------------------------------
@pytest.mark.parametrize("q", [1, 2])
def test_model_gradient_matches_finite_differences(q):
    n = 14
    W = wish_of(count_map(n, seed=4, dead=[5]), "float64")
    X = start(n, W, seed=2)
    _, g = stress_grad(W, X, q)
    h = 1e-6
    fd = numpy.zeros_like(X)
    for i in range(n):
        for c in range(3):
            Xp, Xm = X.copy(), X.copy()
            Xp[i, c] += h
            Xm[i, c] -= h
            fd[i, c] = (stress_grad(W, Xp, q)[0] - stress_grad(W, Xm, q)[0]) / (2 * h)
    assert numpy.all(g[5] == 0.0)                         # the dead bin feels nothing
    assert numpy.abs(fd - g).max() < 1e-6 * numpy.abs(g).max()


@pytest.mark.parametrize("q", [3, -1, 1.5, True])
def test_weight_power_is_validated(q):
    with pytest.raises(ValueError):
        bb.StructureSolver(weight_power=q)


def test_weight_power_defaults_to_raw_stress():
    assert bb.StructureSolver().weight_power == 0
    assert bb.StructureSolver(weight_power=2).weight_power == 2


def test_weighted_steps():
    s = numpy.array([0.0, 2.0, 8.0])
    lr, scale = weighted_steps(s, 3, "float64", "auto", True)
    assert lr == 1.0 / 16.0 and numpy.array_equal(scale, [1.0, 4.0, 1.0])
    assert weighted_steps(s, 3, "float64", 0.25, False) == (0.25, None)
    with pytest.raises(ValueError):
        weighted_steps(numpy.array([2.0 ** 61]), 1, "float32", "auto", False)
    weighted_steps(numpy.array([2.0 ** 61]), 1, "float64", "auto", False)
    with pytest.raises(ValueError):
        weighted_steps(numpy.array([numpy.inf]), 1, "float64", "auto", False)


# --------------------------------------------------------------------------
# GPU
# --------------------------------------------------------------------------
def _engine_run(n, dtype, C, q, x0, k, lr, tiles=None):
    eng = HipEngine(n, dtype, tiles=tiles)
    try:
        eng.set_wish_dense(C, "counts", 3.0)
        eng.set_weight_power(q)
        eng.set_coords(x0)
        eng.iterate(k, lr)
        return eng.get_coords(), eng.stress_history(), eng.iteration_path()[0]
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("q", [1, 2])
@pytest.mark.parametrize("n,dtype,k,path", [
    (300, "float64", 20, "row_owner"), (963, "float64", 10, "row_owner"),
    (300, "float32", 20, "row_owner"), (963, "float32", 20, "row_owner"),
    (5000, "float64", 3, "units"), (5000, "float32", 20, "units")])
def test_weighted_parity(n, dtype, k, path, q):
    tol = 1e-12 if dtype == "float64" else 1e-5
    C = count_map(n, seed=n)
    W = wish_of(C, dtype)
    x0 = start(n, W)
    lr = 1.0 / (2.0 * weights(W, q).sum(1).max())
    X_ref, h_ref = model(W, x0, k, lr, q)
    X, h, got_path = _engine_run(n, dtype, C, q, x0, k, lr)
    assert got_path == path
    assert h.shape == (k,)
    assert numpy.abs(h / h_ref - 1).max() < tol
    assert _rel(X, X_ref) < tol


def _blocked(n, dtype, seed):
    """A blocked-sparse map: the tiles of two diagonal blocks and a band between them."""
    ti_tj, _ = tiles_from_blocks(n, [0, n // 2, n], 300, dtype)
    vw = bb.solver.layout_info(n, dtype)["vw"]
    present = numpy.zeros(((n + vw - 1) // vw,) * 2, dtype=bool)
    present[ti_tj[0], ti_tj[1]] = True
    present |= present.T
    blk = numpy.arange(n) // vw
    C = count_map(n, seed=seed)
    C[~present[blk[:, None], blk[None, :]]] = 0.0
    return ti_tj, C


@pytest.mark.gpu
@pytest.mark.parametrize("q", [1, 2])
@pytest.mark.parametrize("dtype,k", [("float64", 3), ("float32", 20)])
def test_weighted_parity_blocked_sparse(dtype, k, q, monkeypatch):
    monkeypatch.setenv("BB_ROW_OWNER_MAX", "0")            # the blocked unit sweep
    tol = 1e-12 if dtype == "float64" else 1e-5
    n = 2600
    tiles, C = _blocked(n, dtype, seed=7)
    W = wish_of(C, dtype)
    x0 = start(n, W)
    lr = 1.0 / (2.0 * weights(W, q).sum(1).max())
    X_ref, h_ref = model(W, x0, k, lr, q)
    X, h, path = _engine_run(n, dtype, C, q, x0, k, lr, tiles=tiles)
    assert numpy.abs(h / h_ref - 1).max() < tol
    assert _rel(X, X_ref) < tol


@pytest.mark.gpu
@pytest.mark.parametrize("n,path", [(963, "row_owner"), (5000, "units")])
def test_weighted_degree_steps_and_auto_lr(n, path):
    q, k = 2, 12 if n < 2000 else 3
    C = count_map(n, seed=11)
    W = wish_of(C, "float64")
    s_ref = weights(W, q).sum(1)
    eng = HipEngine(n, "float64")
    try:
        eng.set_wish_dense(C, "counts", 3.0)
        eng.set_weight_power(q)
        s = eng.weight_sums()
        assert eng.iteration_path()[0] == path
    finally:
        eng.close()
    assert numpy.abs(s - s_ref).max() <= 1e-12 * s_ref.max()
    assert numpy.abs(s[s_ref > 0] / s_ref[s_ref > 0] - 1).max() < 1e-12
    x0 = start(n, W)
    sol = bb.StructureSolver(n_iter=k, dtype="float64", weight_power=q, degree_steps=True).fit(
        C, init=x0)
    top = s.max()
    assert sol.lr_ == 1.0 / (2.0 * top)
    assert numpy.all(numpy.diff(sol.stress_) <= 0.0)
    scale = numpy.where(s > 0, top / numpy.where(s > 0, s, 1.0), 1.0)
    X_ref, h_ref = model(W, x0, k, sol.lr_, q, scale)
    assert numpy.abs(sol.stress_ / h_ref - 1).max() < 1e-12
    assert _rel(sol.structure_, X_ref) < 1e-12
    # lr='auto' without per-bin steps
    sol = bb.StructureSolver(n_iter=k, dtype="float64", weight_power=q).fit(C, init=x0)
    assert sol.lr_ == 1.0 / (2.0 * top)
    assert numpy.all(numpy.diff(sol.stress_) <= 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_resident_contactmap_and_triples_agree_bit_for_bit(dtype):
    rng = numpy.random.default_rng(8)
    n_bins, res, k = 700, 10000, 6
    bi = rng.integers(0, n_bins, 40000)
    bj = numpy.minimum(n_bins - 1, bi + rng.geometric(0.02, 40000))
    key = numpy.unique(bi * n_bins + bj)
    bi, bj = key // n_bins, key % n_bins
    counts = rng.integers(1, 400, bi.size).astype(float)
    triples = numpy.stack([bi * float(res), bj * float(res), counts], 1)
    x0 = numpy.random.default_rng(1).standard_normal((n_bins + 1, 3)) * 0.3
    cm = bb.ContactMap.from_triples(triples, res, n_bins)
    assert cm.is_resident
    a = bb.StructureSolver(n_iter=k, dtype=dtype, weight_power=2).fit(cm, init=x0)
    b = bb.StructureSolver(n_iter=k, dtype=dtype, weight_power=2).fit_triples(
        triples, res, n_bins, init=x0)
    assert a.lr_ == b.lr_
    assert numpy.array_equal(a.structure_, b.structure_)
    assert numpy.array_equal(a.stress_, b.stress_)
    assert numpy.all(numpy.isfinite(a.structure_))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,tol", [("float64", 1e-12), ("float32", 1e-5)])
def test_fit_many_weighted_matches_single_fits(dtype, tol):
    k = 8
    maps = [count_map(n, seed=n) for n in (300, 700, 1200)]
    inits = [start(C.shape[0], wish_of(C, dtype)) for C in maps]
    many = bb.StructureSolver(n_iter=k, dtype=dtype, weight_power=2, degree_steps=True).fit_many(
        maps, inits=inits)
    for C, x0, X, h, lr in zip(maps, inits, many.structures_, many.stresses_, many.lrs_):
        one = bb.StructureSolver(n_iter=k, dtype=dtype, weight_power=2, degree_steps=True).fit(
            C, init=x0)
        assert abs(lr / one.lr_ - 1) < 1e-14
        assert numpy.abs(h / one.stress_ - 1).max() < tol
        assert _rel(X, one.structure_) < tol


def _set_counts(eng, C):
    eng.set_wish_dense(C, "counts", 3.0)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["one launch", "two launches"])
@pytest.mark.parametrize("dtype,tol", [("float32", 1e-5), ("float64", 1e-12)])
def test_two_ranks_weighted(dtype, tol, form, monkeypatch):
    monkeypatch.setenv("BB_PEER_TIMEOUT_MS", "5000")
    monkeypatch.setenv("BB_PEER_FUSED", "1" if form == "one launch" else "0")
    from tests import _ranks
    n, k, world, q = 1100, 7, 2, 2
    C = count_map(n, seed=21)
    W = wish_of(C, dtype)
    x0 = start(n, W)
    engs = _ranks.peer_ranks(world, n, dtype)
    try:
        sums = []
        for e in engs:
            e.run(_set_counts, C)
            e.set_weight_power(q)
            sums.append(e.weight_sums())
            e.set_coords(x0)
        total = numpy.sum(sums, axis=0)                   # float64, rank order
        lr = 1.0 / (2.0 * total.max())
        for e in engs:
            e.iterate_peer(k, lr)
        got = []
        for e in engs:
            assert e.peer_status() == 0
            got.append((e.get_coords(), e.stress_history()))
    finally:
        for e in engs:
            e.close()
    X1, h1, _ = _engine_run(n, dtype, C, q, x0, k, lr)
    for X, h in got:
        assert numpy.array_equal(X, got[0][0]) and numpy.array_equal(h, got[0][1])
        assert _rel(X, X1) < tol
        assert h.shape == h1.shape and numpy.abs(h / h1 - 1).max() < tol


@pytest.mark.gpu
@pytest.mark.parametrize("n", [300, 1500])
def test_float32_smallest_accepted_wish_distance(n, monkeypatch):
    """fp32, q = 2: a pair at the smallest delta the solver accepts (largest weighted degree
    2^60) gives finite results; one just beyond it is refused before iterating."""
    if n > 1000:
        monkeypatch.setenv("BB_ROW_OWNER_MAX", "0")       # the unit sweep too
    rng = numpy.random.default_rng(5)
    W = numpy.triu(1.0 + rng.random((n, n)), 1)
    W = W + W.T
    tiny = numpy.float32(2.0 ** -30)                       # w = 2^60
    W[3, 4] = W[4, 3] = tiny
    W2 = W.copy()
    W2[3, 4] = W2[4, 3] = numpy.float32(2.0 ** -31)
    # the other pairs of bins 3 and 4 must not push the sum over 2^60: drop them
    for M in (W, W2):
        for b in (3, 4):
            keep = M[b, 7 - b]
            M[b, :] = 0.0
            M[:, b] = 0.0
            M[b, 7 - b] = M[7 - b, b] = keep
    x0 = rng.standard_normal((n, 3))
    s = bb.StructureSolver(n_iter=10, dtype="float32", kind="wish", weight_power=2).fit(W, init=x0)
    assert numpy.all(numpy.isfinite(s.structure_)) and numpy.all(numpy.isfinite(s.stress_))
    assert s.lr_ == 1.0 / (2.0 * 2.0 ** 60)
    with pytest.raises(ValueError):
        bb.StructureSolver(n_iter=10, dtype="float32", kind="wish", weight_power=2).fit(W2, init=x0)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_explicit_weight_power_zero_is_the_default(dtype):
    n = 963
    C = count_map(n, seed=3)
    x0 = start(n, wish_of(C, dtype))
    a = bb.StructureSolver(n_iter=10, dtype=dtype).fit(C, init=x0)
    b = bb.StructureSolver(n_iter=10, dtype=dtype, weight_power=0).fit(C, init=x0)
    assert numpy.array_equal(a.structure_, b.structure_)
    assert numpy.array_equal(a.stress_, b.stress_)
