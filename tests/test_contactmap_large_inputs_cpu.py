"""CPU: the preconditions of tests/test_gpu_contactmap_large.py.  Its tolerances are argued from
properties of its INPUTS and of its host references (tests/_large_maps.py); this file asserts
those properties, so that a change to a generator cannot quietly turn a sharp test into a
blunt one.  Nothing here calls the library."""
import numpy
import pytest

from tests import _large_maps as lm


def test_generators_give_the_bits_of_the_small_size_tests():
    """The Toeplitz form of the decaying maps and the scalar form of the indefinite map's shift
    are, bit for bit, the d x d formulas of tests/test_gpu_parity.py."""
    for d in (1, 2, 255, 513):
        rng = numpy.random.default_rng(d)
        i = numpy.arange(d)
        hic = rng.random((d, d)) * 50.0 / (1.0 + numpy.abs(i[:, None] - i[None, :])) ** 0.8
        hic = hic + hic.T
        neg = rng.standard_normal((d, d))
        neg = neg + neg.T - 3.0 * numpy.sqrt(d) * numpy.outer(numpy.ones(d), numpy.ones(d)) / max(d, 1)
        assert numpy.array_equal(lm.hic_matrix(d), hic)
        assert numpy.array_equal(lm.neg_matrix(d), neg)
        rng = numpy.random.default_rng(d)
        m = rng.random((d, d)) * 40.0 / (1.0 + numpy.abs(i[:, None] - i[None, :])) ** 0.7
        assert numpy.array_equal(lm.corr_matrix(d), m + m.T)


def test_cheap_and_integer_matrices_are_symmetric_and_in_range():
    for d in (1, 255, 256, 257, 1500):
        m = lm.cheap_symmetric(d)
        assert m.dtype == numpy.float64 and m.shape == (d, d)
        assert numpy.array_equal(m, m.T) and m.min() >= 0.0 and m.max() < 1.0
        assert lm.is_symmetric_bitwise(m, block=200)
    m = lm.cheap_symmetric(700)
    m[699, 3] = numpy.nextafter(m[699, 3], 2.0)
    assert not lm.is_symmetric_bitwise(m, block=512)
    rng = numpy.random.default_rng(0)
    dead = numpy.array([0, 5, 299])
    m = lm.integer_symmetric(300, rng, dead)
    x = lm.integer_vector(300, rng)
    assert numpy.array_equal(m, m.T) and numpy.array_equal(m, numpy.rint(m))
    live = numpy.setdiff1d(numpy.arange(300), dead)
    assert m[numpy.ix_(live, live)].min() >= 1 and m.max() < 2 ** 20
    assert not m[dead].any() and not m[:, dead].any()
    assert numpy.array_equal(x, numpy.rint(x)) and numpy.abs(x).max() <= 1024


def test_integer_products_are_exact_in_any_order():
    """|m_ij x_j| < 2^30 and a row has at most 8,193 < 2^14 of them: every partial sum is an
    integer below 2^44, so float64 adds them exactly in any order and `M @ x` of numpy is THE
    answer.  Checked against int64 arithmetic at the largest size's bound and on a sample."""
    assert (2 ** 20 - 1) * 1024 * 8193 < 2 ** 44 < 2 ** 53
    rng = numpy.random.default_rng(1)
    m = lm.integer_symmetric(1500, rng)
    x = lm.integer_vector(1500, rng)
    want = m.astype(numpy.int64) @ x.astype(numpy.int64)
    assert numpy.array_equal(m @ x, want.astype(numpy.float64))
    assert numpy.array_equal((m[:, ::-1] @ x[::-1]), want.astype(numpy.float64))


# ---- eigenvector: the reference's own error and the gap ----------------------------------------
@pytest.mark.parametrize("family", ["hic", "neg"])
@pytest.mark.parametrize("d", [4095, 4096, 4097, 8193])
def test_eigsh_reference_is_accurate_and_the_pair_is_well_separated(d, family):
    """What the 1e-10 on the vector rests on: eigsh's own pair has a long-double residual of a
    few 1e-15 |theta| (asserted: <= 1e-14), and the gap to the second eigenvalue in magnitude is
    0.22 to 0.30 |theta| (asserted: >= 0.2).  A unit vector v with |M v - theta v| <= r is
    within r / gap of the eigenvector (sin of the angle; Davis-Kahan), so eigsh's is within
    5e-14 of the truth and a device pair with residual 1e-12 |theta| within 5e-12 of it: 1e-10
    is not tight for a correct kernel."""
    m = lm.EIGEN_FAMILIES[family](d)
    w, U = lm.eigsh_largest(m, k=2)
    gap = (abs(w[0]) - abs(w[1])) / abs(w[0])
    res, rayleigh = lm.residual_longdouble(m, w[0], U[:, 0])
    print("d=%d %s: theta %.6e gap %.3f eigsh residual %.2e |theta|" % (d, family, w[0], gap,
                                                                       res / abs(w[0])))
    assert gap >= 0.2
    assert res <= 1e-14 * abs(w[0])
    assert abs(rayleigh / w[0] - 1) < 1e-14
    assert (w[0] < 0) == (family == "neg")


def test_filtered_eigen_map_keeps_its_gap():
    """The map of the across-filter eigenvector test: 4,200 bins, 200 of them dead."""
    m, dead = lm.filter_eigen_map()
    live = numpy.setdiff1d(numpy.arange(m.shape[0]), dead)
    assert live.shape[0] == 4000 and (m.sum(axis=0)[live] > 0).all() and not m[dead].any()
    w, U = lm.eigsh_largest(m[numpy.ix_(live, live)], k=2)
    assert (abs(w[0]) - abs(w[1])) / abs(w[0]) >= 0.2
    res, _ = lm.residual_longdouble(m[numpy.ix_(live, live)], w[0], U[:, 0])
    assert res <= 1e-14 * abs(w[0])


# ---- correlation: the sampled-row reference ----------------------------------------------------
def test_sampled_rows_reference_equals_corrcoef():
    """The reference of the two largest correlation sizes against numpy.corrcoef itself where
    that is affordable: equal to a few 1e-16 (asserted: 1e-14), in place or not; the row list
    holds both ends and the block edges."""
    d = 2049
    m = lm.corr_matrix(d)
    rows = lm.sample_rows(d)
    for r in (0, 1, 63, 64, 127, 128, d // 2, d - 129, d - 128, d - 2, d - 1):
        assert r in rows
    assert rows.shape[0] >= 25 and rows.min() == 0 and rows.max() == d - 1
    want = numpy.corrcoef(m)[rows]
    keep = m.copy()
    got = lm.corrcoef_rows(m, rows)
    assert numpy.array_equal(m, keep)
    assert numpy.abs(got - want).max() < 1e-14
    got2 = lm.corrcoef_rows(m, rows, in_place=True)
    assert numpy.array_equal(got, got2) and not numpy.array_equal(m, keep)
    # and on the cheap uniform matrices the two largest sizes use
    c = lm.cheap_symmetric(1500)
    rows = lm.sample_rows(1500)
    assert numpy.abs(lm.corrcoef_rows(c, rows) - numpy.corrcoef(c)[rows]).max() < 1e-14
