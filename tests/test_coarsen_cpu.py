"""CPU: the model of the pooled map (tests/_coarsen_model.py, docs/SPEC.md 2.12) against what a
numpy user would write, the condition that makes the GPU bit tests bite (on the non-integer test
maps another order of summation gives other bits), the two structure helpers of
blueberry_amd/resolution.py, and the argument errors that need no library."""
import numpy
import pytest

import blueberry_amd as bb
from blueberry_amd.datatypes import check_coarsen_args
from tests import _coarsen_model as cm
from tests._util import same_bits

CASES = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 2), (63, 7), (64, 16), (65, 16), (65, 64), (129, 10),
         (129, 100), (257, 5), (257, 257), (257, 258), (1000, 10), (1025, 64)]


@pytest.mark.parametrize("n,k", CASES)
def test_model_equals_the_reshape_sum_on_integer_maps(n, k):
    M = cm.integer_map(n, 100 + n)
    want = cm.reshape_sum(M, n, min(k, n))
    got = cm.pooled(M, n, k)
    assert same_bits(got, want)
    assert got.shape == (cm.n_coarse(n, k) + 1,) * 2
    assert numpy.array_equal(got, got.T) and not got[-1].any() and not got[:, -1].any()
    # every fine pair once: the pooled upper triangle holds the fine upper triangle's total
    assert numpy.triu(got).sum() == numpy.triu(M[:n, :n]).sum()
    mean = cm.pooled(M, n, k, "mean")
    nc = cm.n_coarse(n, k)
    iu = numpy.triu_indices(nc)
    assert same_bits(mean[:nc, :nc][iu], (got[:nc, :nc] / cm.cell_counts(n, min(k, n)))[iu])


@pytest.mark.parametrize("n,k", [(64, 2), (65, 3), (129, 10), (257, 16), (1000, 7), (1025, 40)])
def test_the_two_forms_of_the_model_are_the_same_adds(n, k):
    M = cm.wide_map(n, 7 * n + k)
    a, b = cm.pooled_sums_k2(M, n, k), cm.pooled_sums_cumsum(M, n, k)
    iu = numpy.triu_indices(cm.n_coarse(n, k))
    assert same_bits(a[iu], b[iu])


@pytest.mark.parametrize("n,k", cm.ORDER_CASES)
def test_order_matters_on_the_wide_maps(n, k):
    """The GPU tests compare bits against `pooled` on `wide_map(n, wide_seed(n, k))`: that only
    checks the ORDER if another order gives other bits there (from 63 bins on; a map of three
    bins has too few cells for two orders to differ)."""
    M = cm.wide_map(n, cm.wide_seed(n, k))
    got, other = cm.pooled(M, n, k), cm.reshape_sum(M, n, min(k, n))
    assert got.shape == other.shape and not same_bits(got, other)
    assert numpy.allclose(got, other, rtol=1e-12, atol=0.0)


def test_cell_counts():
    c = cm.cell_counts(7, 3)                    # bins of 3, 3, 1
    assert numpy.array_equal(numpy.triu(c), [[6, 9, 3], [0, 6, 3], [0, 0, 1]])
    assert cm.cell_counts(5, 9)[0, 0] == 15


def test_pixel_list_model_lists_the_cells_that_exist():
    R = 10
    t = numpy.array([[0, 0, 2.0], [10, 30, 0.0], [30, 10, 5.0], [20, 20, 1.5], [40, 0, 9.0], [0, 50, 4.0]])
    got, nc = cm.pooled_triples(t, R, 5, 2)     # bin 5 = n_bins: the last triple is ignored
    assert nc == 3
    # bins: (0,0) (1,3 last wins: 5) (2,2) (0,4) -> coarse (0,0)=2, (0,1)=5, (1,1)=1.5, (0,2)=9
    assert numpy.array_equal(got, [[0, 0, 2.0], [0, 20, 5.0], [0, 40, 9.0], [20, 20, 1.5]])
    zero, _ = cm.pooled_triples(numpy.array([[10.0, 30.0, 0.0]]), R, 5, 2)
    assert numpy.array_equal(zero, [[0, 20, 0.0]])          # a stored zero is a stored cell
    none, nc = cm.pooled_triples(numpy.zeros((0, 3)), R, 5, 2)
    assert none.shape == (0, 3) and nc == 3


# ---- the structure helpers -----------------------------------------------------------------------
def test_coarsen_structure_hand_cases():
    X = numpy.arange(21, dtype=numpy.float64).reshape(7, 3)
    got = bb.coarsen_structure(X, 3)
    assert numpy.array_equal(got, [X[0:3].sum(0) / 3, X[3:6].sum(0) / 3, X[6]])       # ragged last bin
    assert same_bits(bb.coarsen_structure(X, 1), X)
    assert numpy.array_equal(bb.coarsen_structure(X, 8), [((X[0] + X[1] + X[2] + X[3] + X[4] + X[5]) + X[6]) / 7])
    assert bb.coarsen_structure(numpy.zeros((0, 3)), 4).shape == (0, 3)


def test_coarsen_structure_leaves_out_non_finite_rows():
    X = numpy.arange(24, dtype=numpy.float64).reshape(8, 3)
    X[1, 2] = numpy.nan
    X[4] = numpy.inf
    X[5, 0] = numpy.nan
    got = bb.coarsen_structure(X, 2)
    assert numpy.array_equal(got[0], X[0]) and numpy.array_equal(got[1], (X[2] + X[3]) / 2)
    assert numpy.isnan(got[2]).all() and numpy.array_equal(got[3], (X[6] + X[7]) / 2)


@pytest.mark.parametrize("n,k", [(1, 1), (7, 3), (64, 8), (65, 8), (100, 7), (10, 11)])
def test_coarsen_structure_equals_the_model(n, k):
    r = numpy.random.default_rng(n + k)
    X = r.standard_normal((n, 3)) * 2.0 ** r.integers(-8, 9, (n, 1))
    X[r.random(n) < 0.2, 1] = numpy.nan
    assert same_bits(bb.coarsen_structure(X, k), cm.coarsen_structure(X, k))


def test_prolong_structure_hand_cases():
    Xc = numpy.array([[0.0, 0.0, 1.0], [3.0, 6.0, 1.0], [5.0, 10.0, 1.0]])
    got = bb.prolong_structure(Xc, 3, 7)        # centres 1, 4, 6
    assert got.shape == (7, 3)
    assert numpy.array_equal(got[:, 0], [0, 0, 1, 2, 3, 4, 5])        # clamped below the first centre
    assert numpy.array_equal(got[:, 1], [0, 0, 2, 4, 6, 8, 10])
    assert numpy.array_equal(got[:, 2], numpy.ones(7))
    assert same_bits(bb.prolong_structure(Xc, 1, 3), Xc)
    Xn = Xc.copy()
    Xn[1] = numpy.nan                           # skipped: 0 at 1 straight to 5 at 6
    assert numpy.array_equal(bb.prolong_structure(Xn, 3, 7)[:, 0], [0, 0, 1, 2, 3, 4, 5])
    assert numpy.isnan(bb.prolong_structure(numpy.full((3, 3), numpy.nan), 3, 7)).all()
    assert same_bits(bb.prolong_structure(Xn, 3, 7), cm.prolong_structure(Xn, 3, 7))
    with pytest.raises(ValueError, match="rows"):
        bb.prolong_structure(Xc, 3, 10)


@pytest.mark.parametrize("n,k", [(64, 8), (65, 8), (100, 7), (1000, 10)])
def test_prolong_of_coarsen_reproduces_a_linear_structure_away_from_the_ends(n, k):
    """A bin's mean of an exactly linear X is X at the bin's centre, and interpolation between
    centres is exact for a linear X: everything between the first and the last centre comes
    back (to rounding); beyond them the end values hold."""
    i = numpy.arange(n, dtype=numpy.float64)
    X = numpy.stack([2.0 * i + 1.0, -0.5 * i, 0.25 * i - 3.0], axis=1)
    back = bb.prolong_structure(bb.coarsen_structure(X, k), k, n)
    nc = cm.n_coarse(n, k)
    first, last = (k - 1) / 2.0, ((nc - 1) * k + n - 1) / 2.0
    inside = (i >= first) & (i <= last)
    assert inside.sum() >= n - k
    assert numpy.abs(back[inside] - X[inside]).max() <= 8 * 2.0 ** -52 * numpy.abs(X).max()
    coarse = bb.coarsen_structure(X, k)
    assert (back[i < first] == coarse[0]).all() and (back[i > last] == coarse[-1]).all()


# ---- argument errors that need no library ---------------------------------------------------------
@pytest.mark.parametrize("factor", [0, -1, True, False, 2.0, "2", None])
def test_a_bad_factor_is_refused_before_the_library(factor):
    with pytest.raises(ValueError, match="factor"):
        check_coarsen_args(factor, "sum")
    with pytest.raises(ValueError, match="factor"):
        bb.coarsen_structure(numpy.zeros((4, 3)), factor)
    with pytest.raises(ValueError, match="factor"):
        bb.prolong_structure(numpy.zeros((4, 3)), factor, 4)
    cmap = bb.ContactMap.from_matrix(numpy.zeros((5, 5)))
    with pytest.raises(ValueError, match="factor"):
        cmap.coarsen(factor)
    with pytest.raises(ValueError, match="factor"):
        bb.coarsen_triples(numpy.zeros((2, 3)), 10, 4, factor)


@pytest.mark.parametrize("how", ["max", "SUM", None, 0, b"sum"])
def test_a_bad_how_is_refused_before_the_library(how):
    with pytest.raises(ValueError, match="how"):
        check_coarsen_args(2, how)
    cmap = bb.ContactMap.from_matrix(numpy.zeros((5, 5)))
    with pytest.raises(ValueError, match="how"):
        cmap.coarsen(2, how=how)
    with pytest.raises(ValueError, match="how"):
        bb.coarsen_triples(numpy.zeros((2, 3)), 10, 4, 2, how=how)


def test_good_arguments_and_the_exports():
    assert check_coarsen_args(3) == (3, 0) and check_coarsen_args(numpy.int64(1), "mean") == (1, 1)
    for name in ("coarsen_triples", "coarsen_structure", "prolong_structure"):
        assert hasattr(bb, name)
    assert "2.12" in bb.__doc__
