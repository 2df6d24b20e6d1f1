"""SPEC 2.8 without a GPU: the float64 model on closed forms, FitScore's derivations against
direct numpy, and StructureSolver.score through the engine= seam (one process, and two gloo
ranks whose sums are added)."""
import numpy
import pytest

import blueberry_amd as bb
from tests import _score_model as model
from tests._jobs import run_ranks


def _pairs(w, x):
    """(d, delta) of the constrained pairs i < j, straight from the definitions."""
    i, j = numpy.nonzero(numpy.triu(w, 1) > 0)
    return numpy.sqrt(((x[i] - x[j]) ** 2).sum(axis=1)), w[i, j], i, j


# ---- the model on closed forms ---------------------------------------------------------------
def test_model_regular_tetrahedron_has_no_stress():
    x = numpy.array([[1.0, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]])
    edge = numpy.sqrt(8.0)
    w = edge * (1 - numpy.eye(4))
    profile, bins = model.score_sums(w, x)
    s = bb.FitScore(profile, bins)
    assert s.n_pairs == 6 and numpy.array_equal(s.pairs, [0, 3, 2, 1])
    assert numpy.abs(s.stress).max() < 1e-30 and s.normalized_stress < 1e-30
    assert numpy.abs(s.bin_stress).max() < 1e-30 and numpy.array_equal(s.bin_pairs, [3, 3, 3, 3])
    assert numpy.isnan(s.pearson)                      # no variance: every pair is the same
    assert numpy.allclose(s.mean_distance[1:], edge, rtol=1e-15) and numpy.isnan(s.mean_distance[0])


def test_model_uniform_line_has_pearson_one():
    n = 40
    x = numpy.zeros((n, 3))
    x[:, 0] = 0.5 * numpy.arange(n)
    w = 3.0 * numpy.abs(numpy.subtract.outer(numpy.arange(n), numpy.arange(n)))   # delta = 6 d
    s = bb.FitScore(*model.score_sums(w, x))
    assert abs(s.pearson - 1.0) < 1e-12
    k = numpy.arange(1, n)
    assert numpy.array_equal(s.pairs[1:], n - k)
    assert numpy.allclose(s.mean_distance[1:], 0.5 * k, rtol=1e-15)
    assert numpy.allclose(s.mean_wish[1:], 3.0 * k, rtol=1e-15)
    assert numpy.allclose(s.rms_relative_error[1:], 5.0 / 6.0, rtol=1e-14)


def test_model_hand_computed_four_bins():
    """x = 0, 3, 3, 7 on a line; pairs (0,1) delta 1, (0,2) delta 2, (1,2) delta 4 (coincident
    bins: d = 0), (2,3) delta 8; (0,3) and (1,3) absent.  Every number below by hand."""
    x = numpy.zeros((4, 3))
    x[:, 0] = [0, 3, 3, 7]
    w = numpy.zeros((4, 4))
    w[0, 1], w[0, 2], w[1, 2], w[2, 3] = 1, 2, 4, 8
    w = w + w.T
    profile, bins = model.score_sums(w, x)
    # pair: d, delta, (d-delta)^2, /delta, rel^2
    # (0,1) k=1: 3, 1, 4, 4, 4        (1,2) k=1: 0, 4, 16, 4, 1      (2,3) k=1: 4, 8, 16, 2, 0.25
    # (0,2) k=2: 3, 2, 1, 0.5, 0.25
    want = numpy.zeros((4, 9))
    want[1] = [3, 3 + 0 + 4, 1 + 4 + 8, 9 + 0 + 16, 1 + 16 + 64, 3 + 0 + 32, 4 + 16 + 16, 4 + 4 + 2, 4 + 1 + 0.25]
    want[2] = [1, 3, 2, 9, 4, 6, 1, 0.5, 0.25]
    assert numpy.array_equal(profile, want)
    want_bins = numpy.array([[2, 4 + 1, 4 + 0.25], [2, 4 + 16, 4 + 1], [3, 1 + 16 + 16, 0.25 + 1 + 0.25],
                             [1, 16, 0.25]])
    assert numpy.array_equal(bins, want_bins)
    s = bb.FitScore(profile, bins)
    assert s.n_pairs == 4 and numpy.array_equal(s.stress, [37, 10.5, 5.5])
    assert s.normalized_stress == 37.0 / 85.0
    assert s.bin_stress.sum() == 2 * s.stress[0]
    assert numpy.isnan(s.mean_distance[3]) and numpy.isnan(s.mean_wish[0])
    assert numpy.isnan(s.rms_relative_error[3]) and s.pairs[3] == 0 and s.pairs.dtype == numpy.int64
    assert s.rms_relative_error[2] == 0.5 and s.bin_relative[3] == 0.5


def test_model_mask_and_dtype():
    w, x = model.float_case(60)
    full = model.score_sums(w, x)
    mask = numpy.zeros((60, 60), dtype=bool)
    mask[:25] = True
    a, b = model.score_sums(w, x, mask=mask), model.score_sums(w, x, mask=~mask)
    for q in (0, 1):
        assert numpy.allclose(a[q] + b[q], full[q], rtol=1e-14, atol=0)
    assert numpy.array_equal(a[0][:, 0] + b[0][:, 0], full[0][:, 0])
    w32 = model.stored_wish(w, "float32")
    assert (w32 == numpy.triu(w, 1).astype(numpy.float32)).all() and not (w32 == numpy.triu(w, 1)).all()
    assert model.stored_wish(numpy.array([[0, 1e-31], [0, 0]]), "float32")[0, 1] == 0.0
    assert model.stored_wish(numpy.array([[0, 1e-31], [0, 0]]), "float64")[0, 1] == 1e-31


def test_exact_case_is_exact_in_any_order():
    """What the bit-for-bit device tests stand on: on exact_case every sum of the model equals
    the integer sum of its terms in units of 1/64, forwards, backwards and shuffled."""
    w, x = model.exact_case(257)
    profile, bins = model.score_sums(w, x)
    d, delta, i, j = _pairs(w, x)
    res = d - delta
    terms = numpy.stack([numpy.ones_like(d), d, delta, d * d, delta * delta, d * delta, res * res,
                         res * res / delta, (res / delta) ** 2], axis=1)
    units = numpy.rint(terms * 64).astype(numpy.int64)
    assert numpy.array_equal(units / 64.0, terms)
    assert (d == 0).any() and (numpy.bincount(numpy.r_[i, j], minlength=257) == 0).any()
    assert 0.25 < 1.0 - len(d) / (257 * 128.0) < 0.4                  # pairs absent
    k = j - i
    for order in (numpy.arange(len(k)), numpy.arange(len(k))[::-1], numpy.random.default_rng(3).permutation(len(k))):
        for col in range(9):
            exact = numpy.bincount(k[order], weights=None, minlength=257) if col == 0 else None
            ints = numpy.zeros(257, dtype=numpy.int64)
            numpy.add.at(ints, k[order], units[order, col])
            floats = numpy.zeros(257)
            numpy.add.at(floats, k[order], terms[order, col])
            assert numpy.array_equal(floats * 64, ints) and numpy.array_equal(profile[:, col] * 64, ints)
            if exact is not None:
                assert numpy.array_equal(exact, profile[:, 0])
    assert int(units.sum(axis=0).max()) < 2 ** 48


# ---- FitScore against direct numpy -------------------------------------------------------------
def test_fitscore_derivations_against_numpy():
    w, x = model.float_case(150)
    profile, bins = model.score_sums(w, x)
    s = bb.FitScore(profile, bins)
    d, delta, i, j = _pairs(w, x)
    res = d - delta

    def close(a, b):
        return numpy.allclose(a, b, rtol=1e-9, atol=0, equal_nan=True)
    assert s.n_pairs == len(d)
    assert close(s.stress, [(res ** 2).sum(), (res ** 2 / delta).sum(), ((res / delta) ** 2).sum()])
    assert close(s.normalized_stress, (res ** 2).sum() / (delta ** 2).sum())
    assert close(s.pearson, numpy.corrcoef(d, delta)[0, 1])
    k = j - i
    cnt = numpy.bincount(k, minlength=150)
    assert numpy.array_equal(s.pairs, cnt) and s.pairs[0] == 0
    with numpy.errstate(invalid="ignore", divide="ignore"):
        assert close(s.mean_distance, numpy.bincount(k, weights=d, minlength=150) / cnt)
        assert close(s.mean_wish, numpy.bincount(k, weights=delta, minlength=150) / cnt)
        assert close(s.rms_relative_error,
                     numpy.sqrt(numpy.bincount(k, weights=(res / delta) ** 2, minlength=150) / cnt))
        both = numpy.r_[i, j]
        bcnt = numpy.bincount(both, minlength=150)
        assert numpy.array_equal(s.bin_pairs, bcnt)
        assert close(s.bin_stress, numpy.bincount(both, weights=numpy.r_[res, res] ** 2, minlength=150))
        assert close(s.bin_relative, numpy.sqrt(
            numpy.bincount(both, weights=numpy.r_[res / delta, res / delta] ** 2, minlength=150) / bcnt))
    ref = model.derive(profile, bins)
    for name, want in ref.items():
        assert close(getattr(s, name), want), name
    assert "pearson" in repr(s)


def test_fitscore_nan_rules():
    n = 6
    empty = bb.FitScore(numpy.zeros((n, 9)), numpy.zeros((n, 3)))
    assert empty.n_pairs == 0 and numpy.isnan(empty.pearson) and numpy.isnan(empty.normalized_stress)
    assert numpy.isnan(empty.mean_distance).all() and numpy.isnan(empty.rms_relative_error).all()
    assert numpy.isnan(empty.bin_relative).all() and (empty.bin_pairs == 0).all()
    assert numpy.array_equal(empty.stress, [0, 0, 0])
    x = numpy.zeros((n, 3))
    x[:, 0] = numpy.arange(n)
    w = numpy.zeros((n, n))
    w[0, 5] = w[5, 0] = 4.0                                   # one pair: no correlation
    one = bb.FitScore(*model.score_sums(w, x))
    assert one.n_pairs == 1 and numpy.isnan(one.pearson)
    assert numpy.isnan(one.mean_distance[[0, 1, 2, 3, 4]]).all() and one.mean_distance[5] == 5.0
    assert numpy.isnan(one.bin_relative[1:5]).all() and one.bin_relative[0] == 0.25
    with pytest.raises(ValueError):
        bb.FitScore(numpy.zeros((n, 8)), numpy.zeros((n, 3)))
    with pytest.raises(ValueError):
        bb.FitScore(numpy.zeros((n, 9)), numpy.zeros((n + 1, 3)))


# ---- StructureSolver.score through the engine= seam -------------------------------------------
def test_score_through_the_engine_seam():
    w, x = model.float_case(300)
    for dtype in ("float64", "float32"):
        solver = bb.StructureSolver(n_iter=2, dtype=dtype, kind="wish", distributed=False,
                                    engine=model.ScoringOracleEngine)
        got = solver.score(w, structure=x)
        want = model.score_sums(w, x, dtype=dtype)
        assert numpy.array_equal(got.sums, want[0]) and numpy.array_equal(got.bin_sums, want[1])
        assert numpy.array_equal(got.bin_pairs, (model.stored_wish(w + 0, dtype) > 0).sum(axis=0)
                                 + (model.stored_wish(w, dtype) > 0).sum(axis=1))
    # structure=None: the fitted structure_; the score of a fit's start is its first stress
    solver = bb.StructureSolver(n_iter=3, dtype="float64", kind="wish", distributed=False,
                                engine=model.ScoringOracleEngine)
    with pytest.raises(ValueError, match="structure"):
        solver.score(w)
    solver.fit(w, init=x)
    own = solver.score(w)
    assert numpy.array_equal(own.sums, model.score_sums(w, solver.structure_)[0])
    assert abs(solver.score(w, structure=x).stress[0] / solver.stress_[0] - 1) < 1e-12
    assert own.stress[0] < solver.stress_[0]
    # kind='counts': delta = c^(-1/alpha)
    counts = numpy.where(w > 0, numpy.where(w > 0, w, 1.0) ** -3.0, 0.0)
    c = bb.StructureSolver(dtype="float64", kind="counts", alpha=3.0, distributed=False,
                           engine=model.ScoringOracleEngine).score(counts, structure=x)
    assert c.n_pairs == own.n_pairs and abs(c.stress[0] / solver.stress_[0] - 1) < 1e-9


def test_score_argument_validation():
    w, x = model.float_case(20)
    solver = bb.StructureSolver(dtype="float64", kind="wish", distributed=False,
                                engine=model.ScoringOracleEngine)
    with pytest.raises(ValueError, match="shape"):
        solver.score(w, structure=x[:-1])
    with pytest.raises(ValueError, match="shape"):
        solver.score(w, structure=x[:, :2])
    bad = x.copy()
    bad[3, 1] = numpy.nan
    with pytest.raises(ValueError, match="finite"):
        solver.score(w, structure=bad)
    bad[3, 1] = numpy.inf
    with pytest.raises(ValueError, match="finite"):
        solver.score(w, structure=bad)
    with pytest.raises(ValueError, match="square"):
        solver.score(w[:, :-1], structure=x)
    with pytest.raises(ValueError, match="2 bins"):
        solver.score(numpy.zeros((1, 1)), structure=numpy.zeros((1, 3)))

    class NeverMade(object):
        def __init__(self, *a, **k):
            raise AssertionError("the engine was made before the arguments were checked")
    guarded = bb.StructureSolver(dtype="float64", kind="wish", distributed=False, engine=NeverMade)
    with pytest.raises(ValueError):
        guarded.score(w, structure=bad)
    with pytest.raises(ValueError):
        guarded.score(w)


# ---- two gloo ranks: each scores its own units, the sums are added ----------------------------
def _score_worker(rank, world, n):
    w, x = model.exact_case(n)
    s = bb.StructureSolver(dtype="float64", kind="wish", engine=model.ScoringOracleEngine).score(w, structure=x)
    part = model.ScoringOracleEngine(n, "float64", rank=rank, world=world)
    part.set_wish_dense(w, "wish", 3.0)
    return s.sums, s.bin_sums, part.score(x)[0][:, 0].sum()


def test_score_on_two_gloo_ranks_equals_one_process():
    n, world = 300, 2
    results = run_ranks(_score_worker, world, n, timeout=240)
    w, x = model.exact_case(n)
    want = model.score_sums(w, x)
    for sums, bin_sums, own_pairs in results:
        assert numpy.array_equal(sums, want[0]) and numpy.array_equal(bin_sums, want[1])
        assert 0 < own_pairs < want[0][:, 0].sum()              # every rank held a share only
