"""CPU: alpha='auto' (SPEC 2.11) -- the argument forms, the refusals, the update rule, the slope's
errors, and the whole search on the float64 model engine of tests/_alpha_model.py (one process,
and two gloo ranks whose sums are all-reduced)."""
import functools
import math

import numpy
import pytest

import blueberry_amd as bb
from blueberry_amd import solver as S
from tests import _alpha_model as model
from tests._jobs import run_ranks


# ---- 1. the argument forms and the read-backs ---------------------------------------------------
@pytest.mark.parametrize("given,stored", [
    ("auto", ("auto", 3.0, 8, 1e-3)),
    (("auto",), ("auto", 3.0, 8, 1e-3)),
    (("auto", 2), ("auto", 2.0, 8, 1e-3)),
    (("auto", 2.5, 5), ("auto", 2.5, 5, 1e-3)),
    (("auto", 4.0, 3, 1e-2), ("auto", 4.0, 3, 1e-2)),
])
def test_argument_forms_and_read_backs(given, stored):
    s = bb.StructureSolver(alpha=given)
    assert s.alpha == stored and s.alpha_auto
    assert (s.alpha_start, s.alpha_rounds, s.alpha_tol) == stored[1:]
    assert isinstance(s.alpha[1], float) and isinstance(s.alpha[2], int) and isinstance(s.alpha[3], float)


def test_a_float_alpha_is_what_it_was():
    s = bb.StructureSolver(alpha=2)
    assert s.alpha == 2.0 and isinstance(s.alpha, float) and not s.alpha_auto
    assert (s.alpha_start, s.alpha_rounds, s.alpha_tol) == (2.0, None, None)
    assert bb.StructureSolver().alpha == 3.0


@pytest.mark.parametrize("bad", ["Auto", "spectral", ("auto", 0.0), ("auto", -1.0), ("auto", math.inf),
                                 ("auto", 3.0, 0), ("auto", 3.0, 2.5), ("auto", 3.0, True),
                                 ("auto", 3.0, 8, 0.0), ("auto", 3.0, 8, math.nan),
                                 ("auto", 3.0, 8, 1e-3, 1), ("landmark", 3.0), (), 0.0, -3.0,
                                 ("auto", None), ("auto", "3"), ("auto", True), ("auto", 3.0, None),
                                 ("auto", 3.0, "8"), ("auto", 3.0, math.nan), ("auto", 3.0, 8.0),
                                 ("auto", 3.0, 8, None), ("auto", 3.0, 8, "tight")])
def test_bad_alpha_is_refused(bad):
    with pytest.raises(ValueError, match="alpha"):
        bb.StructureSolver(alpha=bad)


# ---- 2. _params and _clone carry the tuple ------------------------------------------------------
def test_params_and_clone_carry_the_tuple():
    s = bb.StructureSolver(alpha=("auto", 2.5, 5), n_iter=7, degree_steps=True)
    assert s._params()["alpha"] == ("auto", 2.5, 5, 1e-3)
    c = s._clone(n_iter=9)
    assert c.alpha == s.alpha and c.n_iter == 9 and c.degree_steps
    assert s._clone(alpha=2.0).alpha == 2.0 and not s._clone(alpha=2.0).alpha_auto


# ---- 3. the refusals ----------------------------------------------------------------------------
def test_refusals_name_their_reason():
    with pytest.raises(ValueError, match="kind='wish'"):
        bb.StructureSolver(alpha="auto", kind="wish")
    for init in ("landmark", ("landmark", 16), ("landmark", 16, 0.5)):
        with pytest.raises(ValueError, match="landmark"):
            bb.StructureSolver(alpha="auto", init=init, degree_steps=True)
    s = bb.StructureSolver(alpha="auto", engine=model.AlphaOracleEngine)
    c = model.complete_map(2.0, n=12)[0]
    with pytest.raises(ValueError, match="shortest_path"):
        s.fit(c, complete="shortest_path")
    with pytest.raises(ValueError, match="shortest_path"):
        s.fit_triples(numpy.array([[0.0, 5.0, 2.0]]), 1, 11, complete="shortest_path")
    with pytest.raises(ValueError, match="fit_many"):
        s.fit_many([c, c])
    with pytest.raises(ValueError, match="alpha_"):
        s.score(c, structure=numpy.zeros((12, 3)))            # before a fit: no alpha_ yet
    from tests._engines import OracleEngine
    with pytest.raises(ValueError, match="engine"):           # an engine without the two passes
        bb.StructureSolver(alpha="auto", engine=OracleEngine).fit(c)


# ---- 4. the update rule on recorded histories ---------------------------------------------------
# (alpha_r, p_r) histories of the float64 probe runs at a true exponent of 4 and of 2, the cases
# that degenerate the secant, and both clips
HISTORIES = [
    [(3.0, 0.807850039)],                                          # first step: alpha / p
    [(3.0, 0.807850039), (3.7135605, 0.948035089)],                # secant
    [(3.0, 1.24408486), (2.41141106, 1.11010993)],
    [(3.0, 0.9), (3.2, 0.9)],                                      # g = 0: alpha / p
    [(3.0, 0.9), (3.2, 0.85)],                                     # g < 0: alpha / p
    [(3.0, 0.9), (3.0, 0.95)],                                     # equal alphas: g not finite
    [(3.0, 0.3)],                                                  # clipped to 2 alpha
    [(3.0, 2.7)],                                                  # clipped to alpha / 2
    [(3.0, 0.99), (3.0001, 0.5)],                                  # a secant far away: 2 alpha
    [(12.0, 0.6)],                                                 # clipped to 16
    [(0.4, 1.9)],                                                  # clipped to 0.25
]


@pytest.mark.parametrize("history", HISTORIES)
def test_update_rule_on_recorded_histories(history):
    got, want = S.next_alpha(history), model.next_alpha(history)
    assert abs(got / want - 1) <= 4 * 2.0 ** -53
    a, p = history[-1]
    assert max(a / 2, 0.25) <= got <= min(2 * a, 16.0)


def test_update_rule_values():
    assert S.next_alpha([(3.0, 0.75)]) == 4.0
    assert S.next_alpha([(3.0, 0.9), (3.2, 0.9)]) == 3.2 / 0.9
    assert S.next_alpha([(3.0, 0.9), (3.2, 0.85)]) == 3.2 / 0.85
    assert S.next_alpha([(3.0, 0.9), (3.0, 0.95)]) == 3.0 / 0.95
    assert S.next_alpha([(3.0, 0.3)]) == 6.0 and S.next_alpha([(3.0, 2.7)]) == 1.5
    assert S.next_alpha([(12.0, 0.6)]) == 16.0 and S.next_alpha([(0.4, 1.9)]) == 0.25
    # the secant: ln p is linear in ln alpha through both points, and zero at the result
    h = [(3.0, 0.8), (3.6, 0.9)]
    g = (math.log(0.9) - math.log(0.8)) / (math.log(3.6) - math.log(3.0))
    assert abs(S.next_alpha(h) - math.exp(math.log(3.6) - math.log(0.9) / g)) < 1e-14


# ---- 5. the slope and its errors ---------------------------------------------------------------
def _totals(u, v, zeros=0):
    return numpy.array([len(u), u.sum(), v.sum(), (u * u).sum(), (v * v).sum(), (u * v).sum(), zeros])


def test_slope_of_a_line_and_its_errors():
    rng = numpy.random.default_rng(3)
    u = rng.normal(size=500)
    v = 0.25 + 0.8 * u + 0.01 * rng.normal(size=500)
    p, a, r, ubar, vbar = S.loglog_slope(_totals(u, v))
    want = numpy.polyfit(u, v, 1)
    assert abs(p - want[0]) < 1e-12 and abs(a - want[1]) < 1e-12
    assert abs(r - numpy.corrcoef(u, v)[0, 1]) < 1e-12 and (ubar, vbar) == (u.sum() / 500, v.sum() / 500)
    mp = model.slope(_totals(u, v))
    assert numpy.allclose([p, a, r, ubar, vbar], mp, rtol=1e-13, atol=0)
    for few in (0, 1, 2):
        with pytest.raises(ValueError, match="fewer than 3"):
            S.loglog_slope(_totals(u[:few], v[:few], zeros=10))
    with pytest.raises(ValueError, match="do not vary"):
        S.loglog_slope(_totals(numpy.full(100, 0.7), v[:100]))           # one count everywhere
    with pytest.raises(ValueError, match="do not vary"):
        S.loglog_slope(_totals(0.7 + 1e-9 * u[:100], v[:100]))          # below the rounding guard
    with pytest.raises(RuntimeError, match="<= 0"):
        S.loglog_slope(_totals(u, -v))
    assert math.isnan(S.loglog_slope(_totals(u, numpy.full(500, 2.0) + 1e-12 * u))[2])   # v constant
    flat = S.loglog_slope(_totals(u[:4], 1.0 + 0.5 * u[:4]))
    assert abs(flat[0] - 0.5) < 1e-12 and abs(flat[2] - 1.0) < 1e-12


def test_totals_add_in_ascending_k():
    prof = numpy.random.default_rng(5).normal(size=(300, 7)) * 10.0 ** numpy.arange(7)
    assert numpy.array_equal(S.loglog_totals(prof), model.totals(prof))
    assert numpy.array_equal(S.loglog_totals(numpy.zeros((0, 7))), numpy.zeros(7))


# ---- 5b. the model's two passes against direct formulas -------------------------------------------
def test_model_sums_and_repower():
    from tests import _score_model as sm
    w, x = sm.exact_case(40)
    prof, bound = model.sums_and_bounds(w, x)
    i, j = numpy.triu_indices(40, 1)
    on = w[i, j] > 0
    d = numpy.sqrt(((x[i] - x[j]) ** 2).sum(axis=1))
    assert prof[:, 6].sum() == (on & (d == 0)).sum() > 0 and prof[:, 0].sum() == (on & (d > 0)).sum()
    use = on & (d > 0)
    assert abs(prof[:, 1].sum() - numpy.log(w[i, j][use]).sum()) < 1e-10
    assert abs(prof[:, 5].sum() - (numpy.log(w[i, j][use]) * numpy.log(d[use])).sum()) < 1e-9
    assert not bound[:, 0].any() and not bound[:, 6].any() and (bound[:, 1:6] >= 0).all()
    stored = numpy.array([0.0, 1e-20, 1e25, 2.0, 0.5])
    assert numpy.array_equal(model.repower(stored, 2.0, "float32"),
                             numpy.array([0.0, 0.0, 0.0, 4.0, 0.25]))       # floor and ceiling
    assert numpy.array_equal(model.repower(stored, 2.0, "float64"), stored * stored)
    half = model.repower(stored, 0.5, "float32")
    assert half[0] == 0 and numpy.array_equal(half[1:], (stored[1:] ** 0.5).astype("float32"))


# ---- 6. the whole loop on the model engine -------------------------------------------------------
N_ITER = 100
AUTO = ("auto", 3.0, 8, 1e-3)
CASES = [("complete", 2.0), ("complete", 4.0), ("sparse", 2.0), ("sparse", 4.0)]


def case_inputs(which, alpha_true):
    """(counts, start or None, solver keywords) of one end-to-end case."""
    if which == "complete":
        return model.complete_map(alpha_true) + ({},)
    return model.sparse_map(alpha_true) + ({"degree_steps": True},)


@functools.lru_cache(maxsize=None)
def model_run(which, alpha_true):
    """The search of tests/_alpha_model.py on one case: made once, never changed."""
    c, start, kw = case_inputs(which, alpha_true)
    if start is None:
        start = numpy.random.default_rng(0).standard_normal((c.shape[0], 3))
    out = model.search(c, start, N_ITER, *AUTO[1:], **kw)
    for a in out.values():
        if isinstance(a, numpy.ndarray):
            a.setflags(write=False)
    return out


@pytest.mark.parametrize("which,alpha_true", CASES)
def test_search_on_the_model_engine(which, alpha_true):
    c, start, kw = case_inputs(which, alpha_true)
    s = bb.StructureSolver(n_iter=N_ITER, dtype="float64", alpha=AUTO, engine=model.AlphaOracleEngine, **kw)
    s.fit(c, init=start)
    err = abs(s.alpha_ / alpha_true - 1)
    print("alpha auto model %s true %g: alpha_ = %.6f, |alpha_/true - 1| = %.3g, rounds = %d"
          % (which, alpha_true, s.alpha_, err, len(s.alpha_rounds_)))
    assert err <= 1e-2 and s.alpha_converged_ and len(s.alpha_rounds_) <= 8
    assert s.alpha_rounds_.shape[1] == 5 and (s.alpha_rounds_[:, 4] == N_ITER).all()
    assert s.alpha_rounds_[0, 0] == 3.0 and s.alpha_rounds_[-1, 0] == s.alpha_
    assert abs(s.alpha_rounds_[-1, 1] - 1) <= 1e-3 and s.alpha_rounds_[-1, 3] > 0.999
    # the product's loop against the model's own
    m = model_run(which, alpha_true)
    assert m["rounds"].shape == s.alpha_rounds_.shape and m["converged"]
    assert numpy.allclose(m["rounds"], s.alpha_rounds_, rtol=1e-9, atol=1e-12)
    assert numpy.allclose(m["init"], s.alpha_init_, rtol=1e-9, atol=1e-12)
    # the fresh-fit identity
    f = bb.StructureSolver(n_iter=N_ITER, dtype="float64", alpha=s.alpha_, engine=model.AlphaOracleEngine, **kw)
    f.fit(c, init=s.alpha_init_)
    assert numpy.array_equal(f.structure_, s.structure_) and numpy.array_equal(f.stress_, s.stress_)
    assert f.alpha_ == s.alpha_ and f.alpha_rounds_.shape == (0, 5) and f.alpha_init_ is None
    assert s.stress_.shape == (N_ITER,) and s.n_iter_ == N_ITER
    # score uses alpha_
    assert s.score(c).n_pairs == f.score(c, structure=s.structure_).n_pairs > 0


def test_last_round_without_convergence():
    c, start, kw = case_inputs("complete", 4.0)
    s = bb.StructureSolver(n_iter=N_ITER, dtype="float64", alpha=("auto", 3.0, 2), engine=model.AlphaOracleEngine)
    s.fit(c)
    assert not s.alpha_converged_ and s.alpha_rounds_.shape == (2, 5)
    assert s.alpha_ == s.alpha_rounds_[1, 0] == 3.0 / s.alpha_rounds_[0, 1]


def test_a_diverged_fit_is_named():
    c = model.complete_map(4.0, n=20)[0]
    s = bb.StructureSolver(n_iter=100, lr=1e3, dtype="float64", alpha="auto", engine=model.AlphaOracleEngine)
    with numpy.errstate(all="ignore"):
        with pytest.raises(RuntimeError, match="diverged in round 0"):
            s.fit(c)


def test_constant_counts_are_refused():
    c = numpy.ones((20, 20)) - numpy.eye(20)
    with pytest.raises(ValueError, match="do not vary"):
        bb.StructureSolver(n_iter=5, dtype="float64", alpha="auto", engine=model.AlphaOracleEngine).fit(c)
    two = numpy.zeros((4, 4))
    two[0, 1] = two[1, 0] = 2.0
    two[2, 3] = two[3, 2] = 3.0
    with pytest.raises(ValueError, match="fewer than 3"):
        bb.StructureSolver(n_iter=5, dtype="float64", alpha="auto", engine=model.AlphaOracleEngine).fit(two)


# ---- 7. two gloo ranks: the sums are all-reduced, every rank takes the same alpha -----------------
def _auto_worker(rank, world):
    c, start, kw = case_inputs("sparse", 4.0)
    s = bb.StructureSolver(n_iter=N_ITER, dtype="float64", alpha=AUTO, engine=model.AlphaOracleEngine, **kw)
    s.fit(c, init=start)
    part = model.AlphaOracleEngine(c.shape[0], "float64", rank=rank, world=world)
    part.set_wish_dense(c, "counts", 3.0)
    return s.alpha_, s.alpha_rounds_, s.structure_, part.loglog(start)[:, 0].sum()


def test_search_on_two_gloo_ranks():
    results = run_ranks(_auto_worker, 2, timeout=240)
    m = model_run("sparse", 4.0)
    pairs = (numpy.triu(case_inputs("sparse", 4.0)[0], 1) > 0).sum()
    assert results[0][0] == results[1][0]                               # the same alpha on every rank
    assert numpy.array_equal(results[0][1], results[1][1]) and numpy.array_equal(results[0][2], results[1][2])
    for alpha, rounds, structure, own in results:
        assert abs(alpha / 4.0 - 1) <= 1e-2 and rounds.shape == m["rounds"].shape
        assert numpy.allclose(rounds, m["rounds"], rtol=1e-9, atol=1e-12)
        assert 0 < own < pairs                                          # every rank held a share only
    assert sum(r[3] for r in results) == pairs
