"""GPU: bb_solver_score / StructureSolver.score (SPEC 2.8) against the float64 model of
tests/_score_model.py.

The main kernel test uses inputs on which every term and every sum is exact in float64
(model.exact_case): the device must then give the model's bits whatever order it sums in, at
every size edge of the three unit shapes.  Float maps are held to the bound of
model.sums_and_bounds; every case prints its largest |err| / bound."""
import functools

import numpy
import pytest

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _exact(n):
    """(wish, x, profile, bins) of the exact case: made once per size, never changed."""
    from tests import _score_model as model
    w, x = model.exact_case(n)
    out = (w, x) + model.score_sums(w, x)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _float(n, dtype, kind):
    """(input matrix, structure, profile, bins, profile bound, bins bound) of the float case."""
    from tests import _score_model as model
    w, x = model.float_case(n)
    if kind == "wish":
        given, delta, extra = w, w, 0.0
    else:
        # counts whose wish distance c^(-1/3) is the walk's, to the rounding of two powers; the
        # device's pow may differ from numpy's: 1e-12 B in fp64 (the project's allowance), and
        # in fp32 delta may differ by one float32 ulp, each term by at most 4 times that
        given = numpy.where(w > 0, numpy.where(w > 0, w, 1.0) ** -3.0, 0.0)
        delta = numpy.where(given > 0, numpy.where(given > 0, given, 1.0) ** (-1.0 / 3.0), 0.0)
        extra = 1e-12 if dtype == "float64" else 2.0 ** -21
    out = (given, x) + model.sums_and_bounds(delta, x, dtype=dtype, extra=extra)
    for a in out:
        a.setflags(write=False)
    return out


def _engine(n, dtype, matrix, kind="wish", **kw):
    from blueberry_amd.solver import HipEngine
    eng = HipEngine(n, dtype, **kw)
    eng.set_wish_dense(matrix, kind, 3.0)
    return eng


def _same_bits(got, want):
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape
    assert numpy.array_equal(got[0], want[0]), numpy.argwhere(got[0] != want[0])[:5]
    assert numpy.array_equal(got[1], want[1]), numpy.argwhere(got[1] != want[1])[:5]


def _within(got, case, label):
    """|device - model| <= bound for all 9 + 3 columns; prints the largest ratio."""
    worst = 0.0
    for dev, ref, bound in ((got[0], case[2], case[4]), (got[1], case[3], case[5])):
        err = numpy.abs(dev - ref)
        assert ((bound > 0) | (err == 0)).all()
        ratio = (err / numpy.where(bound > 0, bound, 1.0)).max(axis=0)
        worst = max(worst, float(ratio.max()))
        assert (err <= bound).all(), (label, ratio)
    print("score %s: max |err| / bound = %.3g" % (label, worst))
    return worst


# ---- 1. exact inputs at every size edge ------------------------------------------------------
EDGES = ([("float32", n) for n in (2, 3, 4, 5, 511, 512, 513, 1025, 1537)]
         + [("float64", n) for n in (2, 7, 8, 9, 127, 128, 129, 257, 4096)]      # 8 x 128 units
         + [("float64", 4097)])                                                    # 2 x 512 units


@pytest.mark.parametrize("dtype,n", EDGES)
def test_exact_inputs_bit_for_bit(dtype, n):
    w, x, profile, bins = _exact(n)
    eng = _engine(n, dtype, w)
    lay = eng.layout()
    assert (lay["vw"], lay["rows_per_unit"]) == (
        (512, 4) if dtype == "float32" else ((128, 8) if n <= 4096 else (512, 2)))
    _same_bits(eng.score(x), (profile, bins))
    assert not profile[0].any() and profile[:, 0].sum() > 0
    eng.set_coords(x)                                 # xyz = NULL: the solver's own, widened
    _same_bits(eng.score(), (profile, bins))
    eng.close()


# ---- 2. blocked-sparse input -------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("n", [1537, 2600])
def test_blocked_sparse_input_bit_for_bit(dtype, n):
    import scipy.sparse
    import blueberry_amd as bb
    from blueberry_amd.solver import layout_info, tiles_from_entries
    from tests import _score_model as model
    w, x = _exact(n)[:2]
    i, j = numpy.indices((n, n))
    band = numpy.where(numpy.abs(i - j) < 600, w, 0.0)
    sp = scipy.sparse.coo_matrix(numpy.triu(band, 1))
    tiles = tiles_from_entries(n, sp.row, sp.col, dtype)
    assert 0 < len(tiles[0]) < layout_info(n, dtype)["n_tiles"]           # some tiles are absent
    solver = bb.StructureSolver(dtype=dtype, kind="wish")
    sparse, dense = solver.score(sp, structure=x), solver.score(band, structure=x)
    want = model.score_sums(band, x)
    _same_bits((sparse.sums, sparse.bin_sums), want)
    _same_bits((dense.sums, dense.bin_sums), want)
    assert sparse.n_pairs == int(want[0][:, 0].sum()) and not sparse.pairs[600:].any()


# ---- 3. float maps -----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["wish", "counts"])
@pytest.mark.parametrize("dtype,n", [("float32", 1537), ("float64", 1537), ("float64", 4097)])
def test_float_map_within_the_bound(dtype, n, kind):
    case = _float(n, dtype, kind)
    eng = _engine(n, dtype, case[0], kind=kind)
    got = eng.score(case[1])
    eng.close()
    assert numpy.array_equal(got[0][:, 0], case[2][:, 0]) and numpy.array_equal(got[1][:, 0], case[3][:, 0])
    assert case[2][:, 6].sum() > 0.1 * case[2][:, 0].sum()               # the residuals do not vanish
    _within(got, case, "%s N=%d %s" % (dtype, n, kind))


# ---- 4. against the sweep ----------------------------------------------------------------------
@pytest.mark.parametrize("q", [0, 1, 2])
@pytest.mark.parametrize("dtype,tol", [("float64", 1e-12), ("float32", 1e-5)])
@pytest.mark.parametrize("n", [4097, 963])                              # unit sweep, row owner
def test_stress_equals_the_sweeps(n, dtype, tol, q):
    import blueberry_amd as bb
    w, y = _float(n, "float64", "wish")[:2]
    if dtype == "float32":
        y = y.astype(numpy.float32).astype(numpy.float64)              # the fit's own start, exactly
    fit = bb.StructureSolver(n_iter=1, weight_power=q, kind="wish", dtype=dtype).fit(w, init=y)
    score = fit.score(w, structure=y)
    print("score vs sweep %s N=%d q=%d: rel %.3g" % (dtype, n, q, abs(score.stress[q] / fit.stress_[0] - 1)))
    assert abs(score.stress[q] / fit.stress_[0] - 1) < tol


# ---- 5. consistency ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_consistency_of_the_two_arrays(dtype):
    import blueberry_amd as bb
    n = 1537
    w, x = _exact(n)[:2]
    eng = _engine(n, dtype, w)
    exact = bb.FitScore(*eng.score(x))
    assert numpy.array_equal(exact.bin_pairs, eng.degrees())
    assert exact.bin_stress.sum() == 2 * exact.stress[0] and exact.bin_pairs.sum() == 2 * exact.n_pairs
    assert (exact.bin_pairs == 0).any() and numpy.isnan(exact.bin_relative[exact.bin_pairs == 0]).all()
    eng.close()
    wf, xf = _float(n, dtype, "wish")[:2]
    eng = _engine(n, dtype, wf)
    a, b = eng.score(xf), eng.score(xf)
    _same_bits(a, b)
    s = bb.FitScore(*a)
    assert numpy.array_equal(s.bin_pairs, eng.degrees())
    assert abs(s.bin_stress.sum() / (2 * s.stress[0]) - 1) < 1e-13
    assert 0.9 < s.pearson < 1.0 and 0 < s.normalized_stress < 0.1
    eng.close()


# ---- 6. the solver's state is untouched ---------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("n", [4097, 963])                              # unit sweep, row owner
def test_score_leaves_the_solver_as_it_was(n, dtype):
    w, x0 = _float(n, "float64", "wish")[:2]
    other = numpy.random.default_rng(9).standard_normal((n, 3))
    scale = 0.5 + 0.5 * numpy.random.default_rng(10).random(n)
    runs = []
    for scored in (True, False):
        eng = _engine(n, dtype, w)
        assert eng.iteration_path()[0] == ("row_owner" if n == 963 else "units")
        eng.set_bin_steps(scale)
        eng.set_coords(x0)
        eng.set_momentum(0.3)
        eng.iterate(3, 0.5 / n)
        if scored:
            mine = eng.score()
            theirs = eng.score(other)
            assert mine[0][:, 6].sum() != theirs[0][:, 6].sum()
        eng.iterate(3, 0.5 / n)
        runs.append((eng.get_coords(), eng.stress_history()))
        eng.close()
    assert runs[0][1].shape == (6,) and numpy.isfinite(runs[0][1]).all() and runs[0][1][5] < runs[0][1][0]
    assert numpy.array_equal(runs[0][0], runs[1][0]) and numpy.array_equal(runs[0][1], runs[1][1])


# ---- 7. several devices from one process ---------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_group_of_three_members(dtype):
    import blueberry_amd as bb
    n = 1537
    w, x, profile, bins = _exact(n)
    grp = bb.StructureSolver(dtype=dtype, kind="wish", devices=[0, 0, 0])
    got = grp.score(w, structure=x)
    _same_bits((got.sums, got.bin_sums), (profile, bins))
    one = bb.StructureSolver(dtype=dtype, kind="wish").score(w, structure=x)
    _same_bits((got.sums, got.bin_sums), (one.sums, one.bin_sums))
    case = _float(n, dtype, "wish")
    got = grp.score(case[0], structure=case[1])
    _within((got.sums, got.bin_sums), case, "%s N=%d group of 3" % (dtype, n))
    # every member held a share of the pairs only
    from blueberry_amd.solver import GroupEngine
    eng = GroupEngine(n, dtype, [0, 0, 0])
    eng.set_wish_dense(w, "wish", 3.0)
    shares = [m.score(x)[0][:, 0].sum() for m in eng.members]
    eng.close()
    assert all(0 < s < profile[:, 0].sum() for s in shares) and sum(shares) == profile[:, 0].sum()


# ---- 8. errors -------------------------------------------------------------------------------------
def test_score_errors():
    import blueberry_amd as bb
    from blueberry_amd import _lib
    from blueberry_amd.solver import HipEngine
    n = 300
    w, x = _exact(n)[:2]
    eng = HipEngine(n, "float32")
    with pytest.raises(RuntimeError, match="no wish distances"):
        eng.score(x)
    eng.set_wish_dense(w, "wish", 3.0)
    with pytest.raises(RuntimeError, match="no coordinates"):
        eng.score()                                               # xyz = NULL before set_coords
    eng.set_coords(x)
    eng.grad()
    with pytest.raises(RuntimeError, match="pending"):
        eng.score(x)
    eng.apply(0.5 / n)
    # non-finite xyz through the C entry (the Python engine refuses it earlier)
    lib = _lib.load()
    profile, bins = numpy.zeros((n, 9)), numpy.zeros((n, 3))
    for bad_value in (numpy.nan, numpy.inf):
        bad = x.copy()
        bad[n - 1, 2] = bad_value
        rc = lib.bb_solver_score(eng._h, _lib.as_f64_ptr(bad), _lib.as_f64_ptr(profile), _lib.as_f64_ptr(bins))
        assert rc == _lib.BB_ERR_INVALID and "finite" in _lib.last_error()
    assert lib.bb_solver_score(eng._h, _lib.as_f64_ptr(x), None, _lib.as_f64_ptr(bins)) == _lib.BB_ERR_INVALID
    before = eng.get_coords()
    assert eng.score(x)[0][:, 0].sum() == _exact(n)[2][:, 0].sum()   # and still works
    assert numpy.array_equal(eng.get_coords(), before) and eng.stress_history().shape == (1,)
    eng.close()
    # a solver of several maps
    m = HipEngine(1024, "float32", tiles=(numpy.array([0, 1], dtype=numpy.int32),
                                          numpy.array([0, 1], dtype=numpy.int32)))
    m.set_maps([0, 512, 1024], [1.0, 1.0])
    with pytest.raises(RuntimeError, match="several maps"):
        m.score(numpy.zeros((1024, 3)))
    m.close()
    # through Python: wrong shape, non-finite structure, no structure_ -- before the device
    solver = bb.StructureSolver(dtype="float32", kind="wish")
    with pytest.raises(ValueError, match="shape"):
        solver.score(w, structure=x[:-1])
    bad = x.copy()
    bad[0, 0] = numpy.nan
    with pytest.raises(ValueError, match="finite"):
        solver.score(w, structure=bad)
    with pytest.raises(ValueError, match="structure"):
        solver.score(w)
    assert solver.fit(w, init=x).score(w).n_pairs == int(_exact(n)[2][:, 0].sum())
