"""No GPU: the float64 model of the spectral start (tests/_spectral_model.py) against what it
stands for, and the preconditions the cases of tests/test_gpu_spectral.py rest on -- that a
product off by the sweep tolerance moves the model's start by little (so 8 x that movement is a
tight bound for the device), that no Ritz value sits near 0 or near another one, that no
residual sits near the stopping tolerance, and that the integer maps keep every partial sum
exact in float32."""
import numpy
import pytest

from tests import _spectral_model as sm


@pytest.mark.parametrize("n", [4, 5, 9, 64, 300])
def test_model_recovers_a_complete_map_after_one_product(n):
    xs, w = sm.walk_map(n, seed=3)
    for op in (sm.dense_op(w), sm.complete_op(xs)):
        got = sm.spectral_ref(op, sm.start_block(n, 1), 1)
        assert got.products == 1 and len(got.residuals) == 2
        assert numpy.abs(sm.pair_distances(got.x0) - w).max() < 1e-9 * w.max()
        assert got.residuals[1] < 1e-6     # in span(V); a difference of sums resolves 1e-8
        assert numpy.abs(got.x0.mean(axis=0)).max() < 1e-9 * numpy.abs(got.x0).max()


@pytest.mark.parametrize("tol", [0.0, 1e-3])
@pytest.mark.parametrize("n", [37, 150, 300])
def test_model_equals_the_host_driven_loop_on_the_oracle_engine(n, tol):
    """solver.spectral_init with the CPU oracle's matvec behind it: same number of products,
    same start, on a map whose loop does run (10 % of the pairs missing)."""
    from blueberry_amd.solver import spectral_init
    from tests._engines import OracleEngine
    w = sm.holed_map(n, seed=n)
    eng = OracleEngine(n, "float64")
    eng.set_wish_dense(w, "wish", 3.0)
    cap = 40 if tol == 0.0 else 80
    x_host, done_host = spectral_init(eng, n, 1, n_iter=cap, seed=4, tol=tol, return_iterations=True)
    got = sm.spectral_ref(sm.dense_op(w), sm.start_block(n, 4), cap, tol)
    assert got.products == done_host
    assert done_host == cap if tol == 0.0 else 1 < done_host <= cap
    assert numpy.abs(got.x0 - x_host).max() < 1e-9 * numpy.abs(x_host).max()


def test_complete_op_equals_the_dense_product():
    n = 300
    xs, w = sm.walk_map(n, seed=2)
    U = numpy.random.default_rng(6).standard_normal((n, 3))
    U -= U.mean(axis=0)
    want = sm.matvec_sq_ref(w, U)
    assert numpy.abs(sm.complete_op(xs)(U) - want).max() < 1e-12 * numpy.abs(want).max()
    V = U + 0.3                                             # the sum(U) term, too
    want = sm.matvec_sq_ref(w, V)
    assert numpy.abs(sm.complete_op(xs)(V) - want).max() < 1e-12 * numpy.abs(want).max()


def test_clean_wish_is_the_packers_rule():
    w = sm.integer_map(40, seed=1)
    m = sm.with_junk(w, seed=1)
    assert (numpy.diag(m) != 0).all() and not numpy.isfinite(numpy.tril(m, -1)).all()
    c = sm.clean_wish(m)
    assert numpy.array_equal(c, c.T) and (numpy.diag(c) == 0).all() and numpy.isfinite(c).all()
    kept = numpy.triu(numpy.isfinite(m) & (m > 0), 1)
    assert numpy.array_equal(numpy.triu(c, 1), numpy.where(kept, m, 0.0))
    assert 0.05 < 1.0 - kept.sum() / numpy.triu(w > 0, 1).sum() < 0.2     # a tenth was junk
    counts = sm.clean_wish(numpy.array([[0.0, 8.0], [numpy.nan, 0.0]]), "counts", 3.0)
    assert numpy.allclose(counts, [[0.0, 0.5], [0.5, 0.0]], rtol=1e-15)


def _separated(ritz, dtype):
    """Every Ritz value at least 100 tol_T lambda_1 away from 0 and from the other two."""
    gap = 100.0 * sm.TOL_T[dtype] * abs(ritz[0])
    others = numpy.abs(ritz[:, None] - ritz[None, :])[~numpy.eye(3, dtype=bool)]
    return numpy.abs(ritz).min() >= gap and others.min() >= gap


@pytest.mark.parametrize("dtype", sm.DTYPES)
@pytest.mark.parametrize("n", sm.SIZES_PRODUCTS)
def test_k_products_cases_are_well_conditioned(n, dtype):
    w, v0 = sm.products_case(n)
    assert numpy.array_equal(w, w.T) and (numpy.diag(w) == 0).all()
    if n >= 63:
        assert 0.05 < (numpy.triu(w == 0, 1).sum() / (n * (n - 1) / 2)) < 0.15
    for k in sm.K_PRODUCTS:
        ref = sm.spectral_ref(sm.dense_op(w), v0, k)
        assert ref.products == k and len(ref.residuals) == k + 1
        m, _ = sm.movement(sm.dense_op(w), v0, k, 0.0, dtype, ref)
        assert 0.0 < m <= 1e-3, (n, k, dtype, m)
        assert _separated(ref.ritz, dtype), (n, k, dtype, ref.ritz)


def test_ill_conditioned_start_block_case():
    """cond(v0) is about 1e6, yet the model's start is that of the well-conditioned block with
    the same span (Householder QR loses cond eps, far below 8 m), m is as small as for any
    other start (with k = 0 only the Rayleigh-Ritz product is perturbed) and the Ritz values
    are apart."""
    w, v0, g = sm.ill_conditioned_case()
    sv = numpy.linalg.svd(v0, compute_uv=False)
    assert 3e5 < sv[0] / sv[-1] < 1e7
    c01 = v0[:, 0] @ v0[:, 1] / numpy.linalg.norm(v0[:, 0]) / numpy.linalg.norm(v0[:, 1])
    assert 1.0 - c01 < 1e-11                                 # the first two columns nearly parallel
    op = sm.dense_op(w)
    ref, plain = sm.spectral_ref(op, v0, 0), sm.spectral_ref(op, g, 0)
    m, _ = sm.movement(op, v0, 0, 0.0, "float32", ref)
    assert 0.0 < m <= 1e-3 and _separated(ref.ritz, "float32")
    assert numpy.abs(ref.x0 - plain.x0).max() <= 1e-3 * 8 * m * numpy.abs(ref.x0).max()


@pytest.mark.parametrize("dtype", sm.DTYPES)
@pytest.mark.parametrize("n,tol", sm.STOP_CASES)
def test_stopping_rule_cases_are_well_conditioned(n, tol, dtype):
    w, v0 = sm.stop_case(n, tol)
    ref = sm.spectral_ref(sm.dense_op(w), v0, sm.STOP_CAP, tol)
    assert 1 < ref.products < sm.STOP_CAP
    m, moved = sm.movement(sm.dense_op(w), v0, sm.STOP_CAP, tol, dtype, ref)
    assert moved.products == ref.products and 0.0 < m <= 1e-3, (n, tol, dtype, m)
    assert _separated(ref.ritz, dtype), (n, tol, dtype, ref.ritz)
    for r in ref.residuals[1:]:                              # the first product is not judged
        assert not tol / 2 <= r <= 2 * tol, (n, tol, ref.residuals)
    assert ref.residuals[-1] < tol and min(ref.residuals[1:-1], default=1.0) >= tol


@pytest.mark.parametrize("n", sm.SIZES_MATVEC + (100, 1300))
def test_integer_maps_keep_every_partial_sum_exact(n):
    w, x = sm.integer_map(n, seed=n), sm.integer_rhs(n, seed=n)
    assert set(numpy.unique(w)) <= {0.0, 1.0, 2.0, 3.0} and numpy.abs(x).max() <= 2
    if n >= 127:
        assert 0.2 < (numpy.triu(w == 0, 1).sum() / (n * (n - 1) / 2)) < 0.3
    assert sm.largest_partial_sum(w, x) < sm.MAX_EXACT
    assert numpy.array_equal(sm.matvec_sq_int(w, x), sm.matvec_sq_ref(w, x))
    c = sm.clean_wish(sm.with_junk(w, seed=n))
    assert sm.largest_partial_sum(c, x) < sm.MAX_EXACT


@pytest.mark.parametrize("n,half", [(1300, 200), (2100, 200), (65600, 40)])
def test_band_maps_keep_every_partial_sum_exact(n, half):
    r, c, v = sm.band_entries(n, half, seed=n)
    assert ((c - r >= 1) & (c - r <= half) & (c < n)).all() and r.size == numpy.unique(r * n + c).size
    assert set(numpy.unique(v)) <= {0.0, 1.0, 2.0, 3.0} and 0.2 < (v == 0).mean() < 0.3
    x = sm.integer_rhs(n, seed=n)
    bound = numpy.zeros((n, 3))
    numpy.add.at(bound, r, (v * v)[:, None] * numpy.abs(x[c]))
    numpy.add.at(bound, c, (v * v)[:, None] * numpy.abs(x[r]))
    assert bound.max() < sm.MAX_EXACT
    if n <= 2100:                                            # the entry form equals the dense one
        w = numpy.zeros((n, n))
        w[r, c] = w[c, r] = v
        assert numpy.array_equal(sm.matvec_sq_int_entries(n, r, c, v, x), sm.matvec_sq_int(w, x))


@pytest.mark.parametrize("n", [3, 4, 64, 300])
@pytest.mark.parametrize("kind", sm.DEGENERATE)
def test_degenerate_maps_have_fewer_than_three_directions(kind, n):
    w, exact = sm.degenerate_map(kind, n)
    assert numpy.array_equal(w, w.T) and (numpy.diag(w) == 0).all() and (w >= 0).all()
    J = numpy.eye(n) - 1.0 / n
    lam = numpy.linalg.eigvalsh(-0.5 * J @ (w * w) @ J)
    scale = max(numpy.abs(lam).max(), 1e-300)
    rank = int((numpy.abs(lam) > 1e-9 * scale).sum())
    assert rank == {"line": 1, "plane": 2, "three_points": 2, "empty": 0, "single_edge": 2}[kind] \
        or (kind == "single_edge" and n == 3 and rank <= 2)
    if exact:
        assert lam.min() > -1e-9 * scale                     # a Euclidean map: B is PSD
        got = sm.spectral_ref(sm.dense_op(w), sm.start_block(n, 0), 2)
        assert numpy.abs(sm.pair_distances(got.x0) - w).max() < 1e-6 * w.max()
