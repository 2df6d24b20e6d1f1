"""GPU: alpha='auto' (SPEC 2.11) -- bb_solver_loglog and bb_solver_repower against the float64 model
of tests/_alpha_model.py at the size edges of the three unit shapes, on blocked-sparse maps and
groups, under the forced 24-bit stream; the search end to end against the model's; and the
fresh-fit identity.  Every bounded case prints its largest |err| / bound."""
import functools

import numpy
import pytest

pytestmark = pytest.mark.gpu

TOL = {"float32": 1e-5, "float64": 1e-12}                 # SPEC 4
# the input-route allowance for a device pow (tests/test_gpu_score.py, test_gpu_input_routes.py):
# 1e-12 in fp64; in fp32 delta may differ by one float32 ulp, a term by at most 4 times that
POW_EXTRA = {"float32": 2.0 ** -21, "float64": 1e-12}


@functools.lru_cache(maxsize=None)
def _exact(n, dtype="float64"):
    """(wish, x, profile, bound) on the exact case of the score tests (absent pairs, lonely bins,
    coincident bins; delta in {1, 2, 4, 8}, integer x): made once per size, never changed."""
    from tests import _alpha_model as model
    from tests import _score_model as sm
    w, x = sm.exact_case(n)
    out = (w, x) + model.sums_and_bounds(w, x, dtype=dtype)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _float(n):
    """(wish, structure) of the score tests' float case."""
    from tests import _score_model as sm
    out = sm.float_case(n)
    for a in out:
        a.setflags(write=False)
    return out


def _engine(n, dtype, matrix, kind="wish", **kw):
    from blueberry_amd.solver import HipEngine
    eng = HipEngine(n, dtype, **kw)
    eng.set_wish_dense(matrix, kind, 3.0)
    return eng


def _within(got, want, bound, label):
    """Columns 0 and 6 bit for bit, columns 1 to 5 within the bound; prints the largest ratio."""
    assert got.shape == want.shape
    assert numpy.array_equal(got[:, 0], want[:, 0]) and numpy.array_equal(got[:, 6], want[:, 6]), label
    err = numpy.abs(got - want)[:, 1:6]
    b = bound[:, 1:6]
    assert ((b > 0) | (err == 0)).all(), label
    ratio = float((err / numpy.where(b > 0, b, 1.0)).max())
    print("loglog %s: max |err| / bound = %.3g" % (label, ratio))
    assert (err <= b).all(), (label, ratio)


# ---- 1. loglog against the model at every size edge ------------------------------------------------
EDGES = ([("float32", n) for n in (2, 3, 4, 5, 511, 512, 513, 1025, 1537)]
         + [("float64", n) for n in (2, 7, 8, 9, 127, 128, 129, 257, 4096, 4097)])


@pytest.mark.parametrize("dtype,n", EDGES)
def test_loglog_at_the_size_edges(dtype, n):
    w, x, profile, bound = _exact(n)
    eng = _engine(n, dtype, w)
    lay = eng.layout()
    assert (lay["vw"], lay["rows_per_unit"]) == (
        (512, 4) if dtype == "float32" else ((128, 8) if n <= 4096 else (512, 2)))
    given = eng.loglog(x)
    _within(given, profile, bound, "%s N=%d xyz given" % (dtype, n))
    assert not profile[0].any() and profile[:, 0].sum() > 0
    if n >= 4:
        assert profile[:, 6].sum() > 0                    # coincident bins: d = 0, counted apart
    eng.set_coords(x)                                     # xyz = NULL: the solver's own, widened
    own = eng.loglog()
    eng.close()
    assert numpy.array_equal(own, given)
    # the counts are the score pass's, less the pairs at distance 0
    from tests import _score_model as sm
    assert numpy.array_equal(profile[:, 0] + profile[:, 6], sm.score_sums(w, x)[0][:, 0])


# ---- 2. other layouts, and the state ---------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("n", [1537, 2600])
def test_loglog_blocked_sparse_and_group(dtype, n):
    import scipy.sparse
    from blueberry_amd.solver import GroupEngine, HipEngine, layout_info, tiles_from_entries
    from tests import _alpha_model as model
    w, x = _exact(n)[:2]
    i, j = numpy.indices((n, n))
    band = numpy.where(numpy.abs(i - j) < 600, w, 0.0)
    profile, bound = model.sums_and_bounds(band, x)
    sp = scipy.sparse.coo_matrix(numpy.triu(band, 1))
    tiles = tiles_from_entries(n, sp.row, sp.col, dtype)
    assert 0 < len(tiles[0]) < layout_info(n, dtype)["n_tiles"]           # some tiles are absent
    dense = _engine(n, dtype, band)
    one = dense.loglog(x)
    dense.close()
    _within(one, profile, bound, "%s N=%d dense, banded" % (dtype, n))
    sparse = HipEngine(n, dtype, tiles=tiles)
    sparse.set_wish_sparse(sp.row, sp.col, sp.data, "wish", 3.0)
    got = sparse.loglog(x)
    again = sparse.loglog(x)
    sparse.close()
    assert numpy.array_equal(got, again)                                  # two calls, the same bits
    assert numpy.array_equal(got[:, (0, 6)], one[:, (0, 6)]) and not got[600:].any()
    _within(got, profile, bound, "%s N=%d blocked-sparse" % (dtype, n))
    for t in (None, tiles):
        grp = GroupEngine(n, dtype, [0, 0, 0], tiles=t)
        if t is None:
            grp.set_wish_dense(band, "wish", 3.0)
        else:
            grp.set_wish_sparse(sp.row, sp.col, sp.data, "wish", 3.0)
        total, total2 = grp.loglog(x), grp.loglog(x)
        shares = [m.loglog(x)[:, 0].sum() for m in grp.members]
        grp.close()
        assert numpy.array_equal(total, total2)
        assert numpy.array_equal(total[:, (0, 6)], one[:, (0, 6)])
        assert all(0 < s < one[:, 0].sum() for s in shares) and sum(shares) == one[:, 0].sum()
        _within(total, profile, bound, "%s N=%d group of 3%s" % (dtype, n, "" if t is None else ", sparse"))


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("n", [4097, 963])                              # unit sweep, row owner
def test_loglog_leaves_the_solver_as_it_was(n, dtype):
    w, x0 = _float(n)
    other = numpy.random.default_rng(9).standard_normal((n, 3))
    runs = []
    for probed in (True, False):
        eng = _engine(n, dtype, w)
        assert eng.iteration_path()[0] == ("row_owner" if n == 963 else "units")
        eng.set_coords(x0)
        eng.set_momentum(0.3)
        eng.iterate(3, 0.5 / n)
        if probed:
            mine, theirs = eng.loglog(), eng.loglog(other)
            assert mine[:, 2].sum() != theirs[:, 2].sum() and mine[:, 0].sum() == theirs[:, 0].sum() > 0
        eng.iterate(3, 0.5 / n)
        runs.append((eng.get_coords(), eng.stress_history()))
        eng.close()
    assert runs[0][1].shape == (6,) and numpy.isfinite(runs[0][1]).all()
    assert numpy.array_equal(runs[0][0], runs[1][0]) and numpy.array_equal(runs[0][1], runs[1][1])


def test_loglog_errors():
    from blueberry_amd import _lib
    from blueberry_amd.solver import HipEngine
    n = 300
    w, x = _exact(n)[:2]
    eng = HipEngine(n, "float32")
    with pytest.raises(RuntimeError, match="no wish distances"):
        eng.loglog(x)
    eng.set_wish_dense(w, "wish", 3.0)
    with pytest.raises(RuntimeError, match="no coordinates"):
        eng.loglog()
    eng.set_coords(x)
    eng.grad()
    with pytest.raises(RuntimeError, match="pending"):
        eng.loglog(x)
    with pytest.raises(RuntimeError, match="pending"):
        eng.repower(2.0)
    eng.apply(0.5 / n)
    out = numpy.zeros((n, 7))
    bad = x.copy()
    bad[3, 1] = numpy.nan
    lib = _lib.load()
    assert lib.bb_solver_loglog(eng._h, _lib.as_f64_ptr(bad), _lib.as_f64_ptr(out)) == _lib.BB_ERR_INVALID
    assert "finite" in _lib.last_error()
    assert lib.bb_solver_loglog(eng._h, _lib.as_f64_ptr(x), None) == _lib.BB_ERR_INVALID
    assert numpy.array_equal(eng.loglog(x)[:, 0], _exact(n)[2][:, 0])    # and still works
    # timing on: the score's three kernels, then loglog's two (no per-bin kernel: exactly 0)
    eng.set_timing(1)
    eng.score(x)
    assert all(t > 0 for t in eng.score_timing())
    eng.loglog(x)
    t = eng.score_timing()
    assert t[0] > 0 and t[1] > 0 and t[2] == 0.0
    eng.close()


# ---- 3. repower on values ----------------------------------------------------------------------------
def _planted(n, p, dtype):
    """The float case; for p = 2 with one pair the floor will flush and one the ceiling will
    (1e-20 and 1e25 in fp32; 1e-200 and 1e200 in fp64)."""
    w = numpy.array(_float(n)[0])
    if p == 2:
        low, high = (1e-20, 1e25) if dtype == "float32" else (1e-200, 1e200)
        w[3, 9] = w[9, 3] = low
        w[5, 12] = w[12, 5] = high
    return w


def _delta_sums(want, dtype):
    """Per separation k: the pairs, sum delta and sum delta^2 of a stored symmetric map, and the
    input-route bound of the two sums, ((pairs + 16) 2^-53 + the pow allowance) times the sum."""
    from tests import _score_model as sm
    n = want.shape[0]
    i, j = numpy.nonzero(numpy.triu(want, 1) > 0)
    k = j - i
    order = numpy.argsort(k, kind="stable")
    k, delta = k[order], want[i, j][order]
    cnt = numpy.bincount(k, minlength=n).astype(numpy.float64)
    s1, s2 = sm._segment_sums(delta, k, n), sm._segment_sums(delta * delta, k, n)
    rel = (cnt + 16) * 2.0 ** -53 + POW_EXTRA[dtype]
    return cnt, (s1, rel * s1), (s2, rel * s2)


@pytest.mark.parametrize("p", [0.5, 0.8, 1.25, 2])
@pytest.mark.parametrize("dtype,n", [("float32", 513), ("float32", 1537), ("float64", 129), ("float64", 4097)])
def test_repower_values(monkeypatch, dtype, n, p):
    """The row-owner path (its matrix is rebuilt from the units) at N = 513 and 129, the unit sweep
    at N = 4,097 and -- the row-owner path switched off, as it is above 4,096 bins -- at the
    fp32 N = 1,537."""
    if n == 1537:
        monkeypatch.setenv("BB_ROW_OWNER_MAX", "0")
    from tests import _alpha_model as model
    from tests import _input_model as im
    from tests import _score_model as sm
    w = _planted(n, p, dtype)
    x = _float(n)[1]
    if dtype == "float32":
        x = x.astype(numpy.float32).astype(numpy.float64)
    stored = sm.stored_wish(w, dtype)
    want = model.repower(stored, p, dtype)
    want = want + want.T
    eng = _engine(n, dtype, w)
    assert eng.iteration_path()[0] == ("row_owner" if n in (513, 129) else "units")
    before = eng.degrees()
    eng.repower(p)
    after = eng.degrees()
    assert numpy.array_equal(after, im.degrees_of(want))                  # exact
    if p == 2:
        assert before[3] - after[3] == 1 and before[12] - after[12] == 1  # floor and ceiling
        assert before.sum() - after.sum() == 4
    else:
        assert numpy.array_equal(before, after)
    # score's sum delta and sum delta^2 within the input-route bound with the pow allowance
    cnt, sum1, sum2 = _delta_sums(want, dtype)
    got = eng.score(x)[0]
    assert numpy.array_equal(got[:, 0], cnt)
    worst = 0.0
    for col, (ref, bound) in ((2, sum1), (4, sum2)):
        err = numpy.abs(got[:, col] - ref)
        ratio = float((err / numpy.where(bound > 0, bound, 1.0)).max())
        assert ((bound > 0) | (err == 0)).all() and (err <= bound).all(), (col, ratio)
        worst = max(worst, ratio)
    for q in (1, 2):
        eng.set_weight_power(q)
        bound = im.weight_sum_bound(want, q, POW_EXTRA[dtype])
        err = numpy.abs(eng.weight_sums() - im.weight_sums_of(want, q))
        assert ((bound > 0) | (err == 0)).all() and (err <= bound).all(), q
        worst = max(worst, float((err / numpy.where(bound > 0, bound, 1.0)).max()))
    eng.set_weight_power(0)
    # the stress equals that of a fresh kind='wish' engine given the model's values
    eng.set_coords(x)
    mine = eng.stress()
    eng.iterate(2, 0.5 / n)                               # and the iteration runs on them
    hist = eng.stress_history()
    eng.close()
    fresh = _engine(n, dtype, want)
    assert fresh.iteration_path()[0] == ("row_owner" if n in (513, 129) else "units")
    fresh.set_coords(x)
    theirs = fresh.stress()
    fresh.iterate(2, 0.5 / n)
    fhist = fresh.stress_history()
    fresh.close()
    print("repower %s N=%d p=%g: sums |err| / bound %.3g, stress rel %.3g"
          % (dtype, n, p, worst, abs(mine / theirs - 1)))
    assert abs(mine / theirs - 1) <= TOL[dtype] and numpy.allclose(hist, fhist, rtol=TOL[dtype], atol=0)
    assert abs(hist[0] / mine - 1) <= TOL[dtype]


def test_repower_refusals():
    import blueberry_amd as bb
    from blueberry_amd.solver import HipEngine
    n = 64
    eng = HipEngine(n, "float64")
    with pytest.raises(RuntimeError, match="no wish distances"):
        eng.repower(2.0)
    eng.set_wish_dense(_exact(n)[0], "wish", 3.0)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="finite and > 0"):
            eng.repower(bad)
    deg = eng.degrees()
    eng.repower(1.0)
    assert numpy.array_equal(eng.degrees(), deg)
    eng.close()
    # anchors set: geodesic rows are no power of anything
    k = numpy.arange(n - 1, dtype=numpy.float64)
    triples = numpy.column_stack([k, k + 1, 1.0 + (k % 3)])
    dev = bb.DeviceTriples(triples, 1, 0)
    try:
        e = HipEngine(n, "float64", tiles=dev.tiles(n, "float64"))
        e.set_wish_triples(dev, "wish", 3.0)
        with dev.shortest_paths(n, [0, 20, 40, 63], kind="wish") as rows:
            e.set_anchors(rows, None, 0.5)
        assert e.anchored
        with pytest.raises(RuntimeError, match="anchors"):
            e.repower(2.0)
        e.set_anchors(None)
        e.repower(2.0)                                    # cleared: allowed again
        e.close()
    finally:
        dev.close()


# ---- 4. repower under the forced 24-bit stream -------------------------------------------------------
def test_repower_under_the_forced_stream(monkeypatch):
    from blueberry_amd.solver import HipEngine
    from tests import _oracle
    from tests.test_gpu_pack24 import _env, _same
    from tests.test_gpu_pack24_paths import LR_A, NA, TILES_A, UNITS_A, _blocks_a, _write_blocks
    blocks = _blocks_a()
    x0 = _oracle.noisy_init(_oracle.random_walk(NA))
    runs = {}
    for on in (1, 0):
        _env(monkeypatch, BB_PACK24=on)
        eng = HipEngine(NA, "float32", tiles=TILES_A)
        try:
            _write_blocks(eng, blocks)
            eng.set_coords(x0)
            first = eng.stress()                          # a sweep: the stream is built here
            built = eng.stream_info()
            eng.repower(0.8)
            eng.iterate(5, LR_A)
            assert eng.iteration_path() == ("units", 0)
            info = eng.stream_info()                      # rebuilt from the new units
            out = {"first": numpy.array([first]), "X": eng.get_coords(), "hist": eng.stress_history()}
            eng.grad()
            eng.sync()
            out["exchange"] = eng.read_exchange()
            runs[on] = out
        finally:
            eng.close()
        if on:
            assert built["packed_units"] == UNITS_A and info["packed_units"] == UNITS_A, (built, info)
        else:
            assert built["packed_units"] == 0 and info["packed_units"] == 0
    assert runs[1]["hist"].shape == (5,) and numpy.isfinite(runs[1]["X"]).all()
    assert runs[1]["hist"][0] != runs[1]["first"][0]     # the map did change
    for key in runs[1]:
        assert _same(runs[1][key], runs[0][key]), key


# ---- 5. end to end -----------------------------------------------------------------------------------
# alpha_rounds_ against the model's: the dtype's tolerance (SPEC 4), relative for an entry above 1
# in magnitude and absolute below it (a_r, r_log and p_r near 1 are compared absolutely).
def _rounds_difference(got, want):
    return numpy.abs(got - want) / numpy.maximum(numpy.abs(want), 1.0)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("which,alpha_true", [("complete", 2.0), ("complete", 4.0), ("sparse", 2.0), ("sparse", 4.0)])
def test_search_end_to_end(which, alpha_true, dtype):
    import blueberry_amd as bb
    from tests.test_alpha_cpu import AUTO, N_ITER, case_inputs, model_run
    c, start, kw = case_inputs(which, alpha_true)
    s = bb.StructureSolver(n_iter=N_ITER, dtype=dtype, alpha=AUTO, **kw).fit(c, init=start)
    err = abs(s.alpha_ / alpha_true - 1)
    m = model_run(which, alpha_true)
    print("alpha auto %s %s true %g: alpha_ = %.6f, |alpha_/true - 1| = %.3g, rounds = %d (model %d)"
          % (dtype, which, alpha_true, s.alpha_, err, len(s.alpha_rounds_), len(m["rounds"])))
    assert err <= 1e-2 and s.alpha_converged_ and len(s.alpha_rounds_) <= 8
    assert s.alpha_rounds_.shape == m["rounds"].shape
    diff = _rounds_difference(s.alpha_rounds_, m["rounds"])
    print("   largest difference to the model's rounds: %.3g (allowed %.3g)" % (diff.max(), TOL[dtype]))
    assert numpy.array_equal(s.alpha_rounds_[:, 4], m["rounds"][:, 4])
    assert (diff <= TOL[dtype]).all(), diff
    assert s.stress_.shape == (N_ITER,) and s.structure_.shape == (c.shape[0], 3)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_search_on_a_group_of_two(dtype):
    import blueberry_amd as bb
    from tests.test_alpha_cpu import AUTO, N_ITER, case_inputs
    c, start, kw = case_inputs("complete", 4.0)
    one = bb.StructureSolver(n_iter=N_ITER, dtype=dtype, alpha=AUTO).fit(c)
    grp = bb.StructureSolver(n_iter=N_ITER, dtype=dtype, alpha=AUTO, devices=[0, 0]).fit(c)
    print("alpha auto group of 2 %s: alpha_ = %.6f (one device %.6f)" % (dtype, grp.alpha_, one.alpha_))
    assert abs(grp.alpha_ / 4.0 - 1) <= 1e-2 and grp.alpha_converged_ and grp.devices_ == [0, 0]
    assert grp.alpha_rounds_.shape == one.alpha_rounds_.shape
    # the members' partial sums are cut differently: the run's own tolerance, as SPEC 4 has it for
    # sharded against single-rank runs
    diff = _rounds_difference(grp.alpha_rounds_, one.alpha_rounds_)
    print("   largest difference to the one-device rounds: %.3g (allowed %.3g)" % (diff.max(), TOL[dtype]))
    assert (diff <= TOL[dtype]).all(), diff
    # every member took the same alpha: a fresh group packed at alpha_ repeats the fit bit for bit
    f = bb.StructureSolver(n_iter=N_ITER, dtype=dtype, alpha=grp.alpha_, devices=[0, 0]).fit(c, init=grp.alpha_init_)
    assert numpy.array_equal(f.structure_, grp.structure_) and numpy.array_equal(f.stress_, grp.stress_)


# ---- 6. the fresh-fit identity ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("route", ["dense", "resident", "triples", "triples_weighted"])
def test_fresh_fit_identity(route, dtype):
    import blueberry_amd as bb
    from tests import _alpha_model as model
    c, start = model.sparse_map(3.5, n=300, seed=2)
    n = c.shape[0]
    i, j = numpy.nonzero(numpy.triu(c, 1))
    triples = numpy.column_stack([i * 1000.0, j * 1000.0, c[i, j]])
    kw = {"n_iter": 20, "dtype": dtype, "degree_steps": True}
    if route == "triples_weighted":
        kw.update(weight_power=2, momentum=0.2)

    def fit(solver, init):
        if route == "dense":
            return solver.fit(c, init=init)
        if route == "resident":
            cm = bb.ContactMap.from_triples(triples, 1000, n - 1, device=0)
            assert cm.is_resident
            return solver.fit(cm, init=init)
        return solver.fit_triples(triples, 1000, n - 1, init=init)

    s = fit(bb.StructureSolver(alpha=("auto", 3.0, 3), **kw), start)
    assert s.alpha_rounds_.shape == (3, 5) and s.alpha_ == s.alpha_rounds_[2, 0] != 3.0
    assert s.alpha_init_.shape == (n, 3) and s.stress_.shape == (20,)
    f = fit(bb.StructureSolver(alpha=s.alpha_, **kw), s.alpha_init_)
    assert f.alpha_ == s.alpha_ and f.alpha_rounds_.shape == (0, 5)
    assert numpy.array_equal(f.structure_, s.structure_) and numpy.array_equal(f.stress_, s.stress_)
    assert f.lr_ == s.lr_
    # score uses alpha_
    a, b = s.score(c), f.score(c)
    assert numpy.array_equal(a.sums, b.sums) and a.n_pairs == len(i)


def test_score_before_a_fit_is_refused():
    import blueberry_amd as bb
    c = numpy.ones((8, 8))
    with pytest.raises(ValueError, match="alpha_"):
        bb.StructureSolver(alpha="auto").score(c, structure=numpy.zeros((8, 3)))
