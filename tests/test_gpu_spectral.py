"""GPU: the spectral start -- the sweep as a matvec (`OP = kOpMatvec2`) and the
N x 3 passes of `bb_solver_spectral_init[_tol]` -- against the float64 model of
tests/_spectral_model.py, which shares no code with the library.  Every tolerance here is one of
three: none (integer maps: every sum is exact in fp32 and fp64 in any order); a bound the suite
already uses on complete noise-free maps (test_spectral_init_recovers_exact_distances: distances
within max(tol, 1e-6) w.max(), coordinates within 10 tol w.max(), tol = 1e-9 / 1e-3); or 8 m,
m being how far the MODEL's start moves when each of its products is off by the sweep tolerance
of the type (1e-12 / 1e-5) -- computed here from the model alone, asserted small in
tests/test_spectral_model_cpu.py.  Each case prints what it measured."""
import functools

import numpy
import pytest

import blueberry_amd as bb
from blueberry_amd import _lib
from blueberry_amd.solver import HipEngine, RankDeficient, layout_info, tiles_from_entries
from tests import _spectral_model as sm
# the fixture lives in the parity module and no conftest.py may be added for it: importing the
# name costs that module's import, which the suite pays anyway
from tests.test_gpu_parity import solver_path                     # noqa: F401

pytestmark = pytest.mark.gpu

NT_BYTES = 240 << 20          # build_indices: non-temporal loads once a rank's units exceed this
UNIT_BYTES = 8192


def _engine(n, dtype, w=None, **kw):
    e = HipEngine(n, dtype, **kw)
    if w is not None:
        e.set_wish_dense(w, "wish", 3.0)
    return e


def _exact(got, want, what):
    """Bit for bit: `got` (float64 from the device) holds the integers of `want` (int64)."""
    bad = numpy.argwhere(got != want.astype(numpy.float64))
    assert bad.size == 0, (what, "%d wrong, first at %s: %r != %d"
                           % (len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])]))


# ---- a. the matvec, exact ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _integer_case(n):
    w, x = sm.integer_map(n, seed=n), sm.integer_rhs(n, seed=n)
    want = sm.matvec_sq_int(w, x)
    for a in (w, x, want):
        a.setflags(write=False)
    return w, x, want


@pytest.mark.parametrize("dtype", sm.DTYPES)
@pytest.mark.parametrize("n", sm.SIZES_MATVEC)
def test_matvec_sq_exact_on_integer_maps(n, dtype, solver_path):
    """Wish distances in {0, 1, 2, 3}, right-hand sides in [-2, 2]: one dropped or doubled pair
    changes an integer.  The tile edges 128 and 512, the row-unit edges, the fp64 narrow / wide
    switch (4,096 / 4,097)."""
    if dtype == "float64":
        assert layout_info(n, dtype)["vw"] == (128 if n <= 4096 else 512)
    w, x, want = _integer_case(n)
    e = _engine(n, dtype, w)
    try:
        _exact(e.matvec_sq(x), want, (n, dtype))
        _exact(e.matvec_sq(x[:, ::-1]), want[:, ::-1], (n, dtype, "second call"))
    finally:
        e.close()


@pytest.mark.parametrize("env", [{"BB_WAVES_PER_CU": "8"}, {"BB_WAVES_PER_CU": "4", "BB_PAIR": "0"},
                                 {"BB_ARITH_DESC": "0"}, {"BB_REDUCE_SLICES": "4"}],
                         ids=["wpcu8", "wpcu4_nopair", "table_desc", "slices4"])
@pytest.mark.parametrize("dtype", sm.DTYPES)
@pytest.mark.parametrize("n", [1025, 4097])
def test_matvec_sq_exact_under_the_sweep_switches(n, dtype, env, monkeypatch):
    """The run-time variants of the sweep and its reduce, set as
    test_sweep_and_reduce_variants_vs_oracle sets them.  (No switch reaches the non-temporal
    loads: the 65,600-bin band below does, by size.)"""
    monkeypatch.setenv("BB_ROW_OWNER_MAX", "0")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    w, x, want = _integer_case(n)
    e = _engine(n, dtype, w)
    try:
        _exact(e.matvec_sq(x), want, (n, dtype, env))
    finally:
        e.close()


@pytest.mark.parametrize("dtype", sm.DTYPES)
@pytest.mark.parametrize("n", [9, 129, 513, 1025])
def test_matvec_sq_exact_on_input_with_junk(n, dtype):
    """A non-zero diagonal, NaN / +-inf / negative values in a tenth of the pairs and in the
    whole lower triangle: the product is that of the cleaned upper triangle."""
    w, x, _ = _integer_case(n)
    m = sm.with_junk(w, seed=n)
    want = sm.matvec_sq_int(sm.clean_wish(m), x)
    e = _engine(n, dtype, m)
    try:
        _exact(e.matvec_sq(x), want, (n, dtype))
    finally:
        e.close()


@pytest.mark.parametrize("dtype", sm.DTYPES)
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("n", [100, 1300])
def test_matvec_sq_rank_shares_sum_exactly(n, world, dtype):
    """The ranks' products add up to the whole.  n = 100 is one tile whose row units beyond
    bin 100 hold padding only: in fp32 (128 units of 4 rows) the last rank owns no pair at all."""
    w, x, want = _integer_case(n)
    got, last = numpy.zeros_like(x), None
    for rank in range(world):
        e = _engine(n, dtype, w, rank=rank, world=world)
        try:
            last = e.matvec_sq(x)
            got += last
        finally:
            e.close()
    _exact(got, want, (n, world, dtype))
    if n == 100 and dtype == "float32":
        assert not last.any()


@pytest.mark.parametrize("n,dtype,vw", [(1300, "float64", 128), (2100, "float32", 512)])
def test_matvec_sq_exact_on_a_blocked_sparse_band(n, dtype, vw):
    """A band of +-200 bins through set_wish_sparse: most tiles are absent."""
    assert layout_info(n, dtype)["vw"] == vw
    r, c, v = sm.band_entries(n, 200, seed=n)
    x = sm.integer_rhs(n, seed=n)
    flip = numpy.arange(r.size) % 3 == 0                    # entries may sit in either triangle
    rows, cols = numpy.where(flip, c, r), numpy.where(flip, r, c)
    tiles = tiles_from_entries(n, rows, cols, dtype)
    nb = -(-n // vw)
    assert len(tiles[0]) < nb * (nb + 1) // 2
    e = HipEngine(n, dtype, tiles=tiles)
    try:
        e.set_wish_sparse(rows, cols, v, "wish", 3.0)
        _exact(e.matvec_sq(x), sm.matvec_sq_int_entries(n, r, c, v, x), (n, dtype))
    finally:
        e.close()


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_matvec_sq_exact_on_a_band_of_65600_bins(dtype):
    """Above 65,536 padded bins, a band of +-40 bins on the tiles of the diagonal and the one
    beside it, the engine built as test_genome_10kb_sized_blocked_band_properties builds its
    own.  The units exceed 240 MiB: this is the sweep with non-temporal loads."""
    n, vw = 65600, 512
    nb = -(-n // vw)
    tj, ti = numpy.meshgrid(numpy.arange(nb), numpy.arange(nb))
    sel = (ti <= tj) & (tj - ti <= 1)
    order = numpy.lexsort((ti[sel], tj[sel]))
    tiles = (ti[sel][order].astype(numpy.int32), tj[sel][order].astype(numpy.int32))
    r, c, v = sm.band_entries(n, 40, seed=n)
    x = sm.integer_rhs(n, seed=n)
    e = HipEngine(n, dtype, tiles=tiles)
    try:
        lay = e.layout()
        assert lay["vw"] == vw and lay["n_pad"] > 65536 and lay["n_tiles"] == 2 * nb - 1
        assert lay["n_units"] * UNIT_BYTES > NT_BYTES
        e.set_wish_sparse(r, c, v, "wish", 3.0)
        _exact(e.matvec_sq(x), sm.matvec_sq_int_entries(n, r, c, v, x), (n, dtype))
    finally:
        e.close()


# ---- b. k products against the model -----------------------------------------------------------
@pytest.mark.parametrize("dtype", sm.DTYPES)
@pytest.mark.parametrize("n", sm.SIZES_PRODUCTS)
def test_k_products_equal_the_model(n, dtype):
    """A random walk with 10 % of its pairs removed, k = 0, 1, 3 products (tol = 0): the
    start within 8 m of the model's, centred (once a product has been made), its columns
    orthogonal; the same bits from a second run and from bb_solver_spectral_init.  Sizes: one
    workgroup of the passes and several, one to four waves of real rows, the stride of
    gram3_kernel, a ragged last workgroup everywhere."""
    w, v0 = sm.products_case(n)
    op = sm.dense_op(w)
    lib = _lib.load()
    e = _engine(n, dtype, w)
    try:
        for k in sm.K_PRODUCTS:
            ref = sm.spectral_ref(op, v0, k)
            m, _ = sm.movement(op, v0, k, 0.0, dtype, ref)
            assert e.spectral_init_device(k, v0) == (k, -1.0)
            x = e.get_coords()
            top = numpy.abs(ref.x0).max()
            err = numpy.abs(x - ref.x0).max() / top
            mean = numpy.abs(x.mean(axis=0)).max() / top
            g = x.T @ x
            off = numpy.abs(g - numpy.diag(numpy.diag(g))).max() / ref.ritz[0]
            print("k-products n=%d %s k=%d: err %.2e  m %.2e  err/m %.2f  mean %.1e  offdiag %.1e"
                  % (n, dtype, k, err, m, err / m, mean, off))
            assert numpy.isfinite(x).all()
            assert err <= 8 * m, (n, dtype, k, err, m)
            if k > 0:                            # (k = 0: V = qr(v0) is not centred, nor is the model's)
                assert mean <= 8 * m, (n, dtype, k, mean, m)
            assert off <= 8 * m, (n, dtype, k, off, m)
            assert e.spectral_init_device(k, v0) == (k, -1.0)
            assert numpy.array_equal(e.get_coords(), x)
            _lib.check(lib.bb_solver_spectral_init(e._h, k, _lib.as_f64_ptr(v0)), "bb_solver_spectral_init")
            assert numpy.array_equal(e.get_coords(), x)
    finally:
        e.close()


def test_ill_conditioned_start_block_needs_both_cholesky_qr_passes():
    """The start needs V ORTHONORMAL, not only its span: the Rayleigh-Ritz step takes sym(V'Z)
    for the matrix of B on span(V), and X0 = V E sqrt(lambda).  The library orthonormalises by
    Cholesky-QR twice because one pass leaves cond^2 eps unorthogonal.  The products of a
    healthy map are too well conditioned to show that, but v0 goes through the same two passes
    and is the test's own: cond(v0) = 1e6, the first two columns nearly parallel, k = 0, fp32
    (in fp64 two passes of Cholesky-QR and Householder QR themselves differ by cond eps, above
    that type's 8 m).  m does not feel the conditioning of v0: with k = 0 only the
    Rayleigh-Ritz product is perturbed."""
    dtype = "float32"
    w, v0, _ = sm.ill_conditioned_case()
    op = sm.dense_op(w)
    ref = sm.spectral_ref(op, v0, 0)
    m, _ = sm.movement(op, v0, 0, 0.0, dtype, ref)
    e = _engine(sm.ILL_N, dtype, w)
    try:
        assert e.spectral_init_device(0, v0) == (0, -1.0)
        x = e.get_coords()
    finally:
        e.close()
    err = numpy.abs(x - ref.x0).max() / numpy.abs(ref.x0).max()
    g = x.T @ x
    off = numpy.abs(g - numpy.diag(numpy.diag(g))).max() / ref.ritz[0]
    print("ill-conditioned v0 n=%d %s k=0: err %.2e  offdiag %.2e  m %.2e" % (sm.ILL_N, dtype, err, off, m))
    assert err <= 8 * m and off <= 8 * m, (err, off, m)


# ---- c. the group fold and the row loop, on complete maps ---------------------------------------
def _sampled_pairs(n, count, seed=0):
    rng = numpy.random.default_rng(seed)
    i, j = rng.integers(0, n, count), rng.integers(0, n, count)
    i, j = numpy.concatenate([i, numpy.arange(n - 1)]), numpy.concatenate([j, numpy.arange(1, n)])
    return i, j


def _dist(x, i, j):
    return numpy.sqrt(((x[i] - x[j]) ** 2).sum(axis=1))


@pytest.mark.parametrize("dtype", sm.DTYPES)
@pytest.mark.parametrize("n", [4095, 4096, 4097])
def test_complete_map_where_the_group_fold_wraps(n, dtype):
    """The passes hand 16, 16 and 18 partial sums on (both types pad 4,097 bins to 4,608; 17
    cannot be had), so at 4,097 the 16-lane fold of sp_map_from_partials wraps.  A complete
    noise-free map is exact after one product."""
    lay = layout_info(n, dtype)
    groups = -(-lay["n_pad"] // 256)
    assert groups == (16 if n <= 4096 else 18)
    xs, w = sm.walk_map(n, seed=n)
    v0 = sm.start_block(n, seed=n)
    tol = sm.TOL_EXACT[dtype]
    ref = sm.spectral_ref(sm.complete_op(xs), v0, 2)
    e = _engine(n, dtype, w)
    try:
        assert e.spectral_init_device(2, v0) == (2, -1.0)
        x = e.get_coords()
    finally:
        e.close()
    err_d = numpy.abs(sm.pair_distances(x) - w).max() / w.max()
    err_x = numpy.abs(x - ref.x0).max() / w.max()
    print("complete n=%d %s groups=%d: distances %.2e  coords %.2e (of w.max)" % (n, dtype, groups, err_d, err_x))
    assert err_d < max(tol, 1e-6) and err_x < 10 * tol


def test_complete_map_of_65600_bins_second_trip_of_the_row_loops():
    """n_pad = 66,048 rows for 256 workgroups: 258 rows each, so the strided loops of
    sp_stats_kernel and sp_affine_stats_kernel make a second trip, and every workgroup of every
    pass folds 256 partials.  fp32, 8.6 GB of units made from the coordinates on the device;
    the reference is the model on the closed form of the product.  Distances are checked on
    200,000 random pairs and every pair (i, i + 1)."""
    n, dtype = 65600, "float32"
    tol = sm.TOL_EXACT[dtype]
    xs, v0 = sm.random_walk(n, seed=n), sm.start_block(n, seed=n)
    assert -(-layout_info(n, dtype)["n_pad"] // 256) > 256
    ref = sm.spectral_ref(sm.complete_op(xs), v0, 2)
    i, j = _sampled_pairs(n, 200000)
    want = _dist(xs, i, j)
    # w.max(): the diameter of the walk is attained on the extreme points of a few directions
    # at most; a lower bound makes the bounds below tighter, never wider
    dirs = numpy.random.default_rng(1).standard_normal((256, 3))
    ext = numpy.unique(numpy.concatenate([(xs @ dirs.T).argmax(axis=0), (xs @ dirs.T).argmin(axis=0)]))
    wmax = sm.pair_distances(xs[ext]).max()
    assert wmax >= want.max()
    e = HipEngine(n, dtype)
    try:
        e.set_wish_from_coords(xs)
        assert e.spectral_init_device(2, v0) == (2, -1.0)
        x2 = e.get_coords()
        done, res = e.spectral_init_device(40, v0, tol=1e-3)
        xt = e.get_coords()
    finally:
        e.close()
    # the k = 2 run against the model as the k-products cases are: within 8 m, and centred (a
    # mean taken over a part of the rows leaves a constant column offset, which no distance sees)
    m, _ = sm.movement(sm.complete_op(xs), v0, 2, 0.0, dtype, ref)
    top = numpy.abs(ref.x0).max()
    err, mean = numpy.abs(x2 - ref.x0).max() / top, numpy.abs(x2.mean(axis=0)).max() / top
    print("complete n=%d %s k=2: err %.2e  mean %.2e  m %.2e (of max |X0|)" % (n, dtype, err, mean, m))
    assert err <= 8 * m and mean <= 8 * m, (err, mean, m)
    for name, x in (("k=2", x2), ("tol=1e-3", xt)):
        err_d = numpy.abs(_dist(x, i, j) - want).max() / wmax
        err_x = numpy.abs(x - ref.x0).max() / wmax
        print("complete n=%d %s %s: distances %.2e  coords %.2e (of w.max)" % (n, dtype, name, err_d, err_x))
        assert err_d < max(tol, 1e-6) and err_x < 10 * tol, (name, err_d, err_x)
    print("complete n=%d %s tol=1e-3: %d product(s) orthonormalised, residual %.2e" % (n, dtype, done, res))
    assert done == 1 and 0.0 <= res < 1e-3


# ---- d. the stopping rule against the model ----------------------------------------------------
@pytest.mark.parametrize("dtype", sm.DTYPES)
@pytest.mark.parametrize("n,tol", sm.STOP_CASES)
def test_stopping_rule_equals_the_model(n, tol, dtype):
    w, v0 = sm.stop_case(n, tol)
    op = sm.dense_op(w)
    ref = sm.spectral_ref(op, v0, sm.STOP_CAP, tol)
    m, _ = sm.movement(op, v0, sm.STOP_CAP, tol, dtype, ref)
    e = _engine(n, dtype, w)
    try:
        done, res = e.spectral_init_device(sm.STOP_CAP, v0, tol=tol)
        x = e.get_coords()
    finally:
        e.close()
    err = numpy.abs(x - ref.x0).max() / numpy.abs(ref.x0).max()
    print("stopping n=%d tol=%g %s: products %d (model %d)  residual %.6e (model %.6e)  err %.2e  m %.2e"
          % (n, tol, dtype, done, ref.products, res, ref.residuals[-1], err, m))
    assert abs(done - ref.products) <= (0 if dtype == "float64" else 1)
    assert 0.0 <= res < tol
    if done == ref.products:
        assert abs(res - ref.residuals[-1]) <= 8 * m
        assert err <= 8 * m


# ---- e. maps without three directions ------------------------------------------------------------
def _degenerate_bound(dtype):
    return max(sm.TOL_EXACT[dtype], 1e-6)


@pytest.mark.parametrize("dtype", sm.DTYPES)
@pytest.mark.parametrize("n", [3, 4, 64, 300])
@pytest.mark.parametrize("kind", sm.DEGENERATE)
def test_rank_deficient_maps_on_the_device(kind, n, dtype):
    """B has rank below 3: the third pivot of the Cholesky factor is rounding residue of either
    sign, so the device form either raises RankDeficient or goes on -- both are meant to be
    harmless.  Never another error, never non-finite coordinates; where it returns a start
    after at least one product on a Euclidean map (a line, a plane, three places) the start
    reproduces the map.  (Without a product, k = 0, the start is the Rayleigh-Ritz step on the
    random block itself: exact only where that block spans everything, n = 3.)"""
    w, exact = sm.degenerate_map(kind, n)
    v0 = sm.start_block(n, seed=0)
    e = _engine(n, dtype, w)
    try:
        for k in (0, 2):
            try:
                e.spectral_init_device(k, v0)
                outcome = "continued"
            except RankDeficient:
                outcome = "raised"
            if outcome == "continued":
                x = e.get_coords()
                assert numpy.isfinite(x).all(), (kind, n, dtype, k)
                if exact and (k > 0 or n == 3):
                    err = numpy.abs(sm.pair_distances(x) - w).max() / w.max()
                    outcome += " (distances %.1e)" % err
                    assert err < _degenerate_bound(dtype), (kind, n, dtype, k, err)
            print("degenerate %s n=%d %s k=%d: %s" % (kind, n, dtype, k, outcome))
            e.set_coords(v0)
            e.iterate(1, 1.0 / (2 * n))
            h = e.stress_history()
            assert h.shape == (1,) and numpy.isfinite(h).all() and numpy.isfinite(e.get_coords()).all()
    finally:
        e.close()


@pytest.mark.parametrize("dtype", sm.DTYPES)
@pytest.mark.parametrize("n", [3, 4, 64, 300])
@pytest.mark.parametrize("kind", sm.DEGENERATE)
def test_rank_deficient_maps_through_fit(kind, n, dtype, solver_path):
    w, exact = sm.degenerate_map(kind, n)
    s = bb.StructureSolver(n_iter=1, dtype=dtype, kind="wish", init="spectral").fit(w)
    assert s.structure_.shape == (n, 3) and numpy.isfinite(s.structure_).all()
    assert s.stress_.shape == (1,) and numpy.isfinite(s.stress_).all()
    if not exact:
        return
    if dtype == "float64":
        rnd = bb.StructureSolver(n_iter=1, dtype=dtype, kind="wish", init="random").fit(w)
        print("degenerate fit %s n=%d %s: stress %.3e (random start %.3e)" % (kind, n, dtype, s.stress_[0], rnd.stress_[0]))
        assert s.stress_[0] < 1e-6 * rnd.stress_[0]
    else:
        err = numpy.abs(sm.pair_distances(s.structure_) - w).max() / w.max()
        print("degenerate fit %s n=%d %s: distances %.2e" % (kind, n, dtype, err))
        assert err < _degenerate_bound(dtype)
