"""CPU: what `ContactMap.balance` / `ContactMap.expected` check before they touch a device, and the
properties of the numpy model (tests/_balance_model.py) that tests/test_gpu_balance.py rests on:
the model recovers a planted bias in closed form, and on the Hi-C-like generator it stops clear
of `tol`, so that the device may be asked for the same number of updates.

Every toleranced figure is printed before it is asserted (`pytest -s`)."""
import numpy
import pytest

import blueberry_amd as bb
from tests import _balance_model as bm


def small_map(n=6, **kw):
    m = numpy.zeros((n + 1, n + 1))
    m[:n, :n] = 1.0 + numpy.add.outer(numpy.arange(n), numpy.arange(n))
    return bb.ContactMap.from_matrix(m, **kw)


# ---- 1. argument errors, with no device -----------------------------------------------------------
@pytest.mark.parametrize("kwargs", [
    {"ignore_diags": -1}, {"min_nnz": -1}, {"tol": -1e-9}, {"tol": float("nan")},
    {"tol": float("inf")}, {"max_iter": -1}, {"row_sum": 0.0}, {"row_sum": -2.0},
    {"row_sum": float("inf")}])
def test_balance_refuses_bad_arguments_before_the_device(kwargs):
    cm = small_map()
    with pytest.raises(ValueError):
        cm.balance(**kwargs)
    assert not cm.is_resident and cm._KRnorm is None


@pytest.mark.parametrize("bias", [numpy.ones(5), numpy.ones(7), numpy.ones((6, 1)), "rao"])
def test_expected_refuses_a_bias_of_the_wrong_length(bias):
    cm = small_map()
    with pytest.raises(ValueError):
        cm.expected(bias=bias)
    assert not cm.is_resident and cm._KRexpected is None


def test_expected_auto_refuses_a_short_krnorm():
    cm = small_map(KRnorm=numpy.ones(4))
    with pytest.raises(ValueError):
        cm.expected()
    assert not cm.is_resident


def test_stale_shape_is_refused_with_normalize_s_message():
    """The `keep_stale` case: n_bins no longer matches the matrix."""
    cm = small_map()
    cm.n_bins = 4
    for call in (cm.balance, cm.expected):
        with pytest.raises(ValueError, match="matrix shape does not match n_bins"):
            call()
    assert not cm.is_resident


def test_expected_from_sums_is_never_zero():
    from blueberry_amd.datatypes import expected_from_sums
    e = expected_from_sums(numpy.array([6.0, 0.0, 5.0, 0.0]), numpy.array([3, 4, 0, 0]))
    assert e[0] == 2.0 and numpy.isnan(e[1:]).all()


# ---- 2. the model against a closed form -------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 257])
def test_model_recovers_a_planted_bias_on_a_circulant_decay(n):
    """M_ij = p_i p_j C_ring(i, j): every row of the circulant C has the same sum, so C is
    balanced already and b is a multiple of p.  Every cell of diagonal k lies at the ring
    distance min(k, n - k), so the expected of the balanced map is one multiple of C there."""
    m, p, c = bm.circulant_planted(n, n)
    r = bm.balance(m, tol=1e-28, max_iter=1000)
    ratio = r["bias"] / p
    spread = ratio.max() / ratio.min() - 1.0
    print("n=%d: %d updates, var %.2e, spread of b / p %.2e" % (n, r["iterations"], r["variance"], spread))
    assert r["converged"] and not r["masked"].any()
    assert spread < 1e-12
    sums, counts, e = bm.expected(m, r["bias"])
    assert numpy.array_equal(counts, n - numpy.arange(n))
    k = numpy.arange(n)
    ring = numpy.minimum(k, n - k)
    scale = e / c[ring]
    spread_e = scale.max() / scale.min() - 1.0
    print("n=%d: spread of e_k / C_k %.2e" % (n, spread_e))
    assert spread_e < 1e-12
    # row_sum=1.0 is cooler's convention: the balanced rows sum to 1
    r1 = bm.balance(m, tol=1e-28, max_iter=1000, row_sum=1.0)
    a = bm.counted_cells(m) / numpy.outer(r1["bias"], r1["bias"])
    assert numpy.abs(a.sum(axis=1) - 1.0).max() < 1e-12


def test_model_mask_reaches_its_fixed_point():
    """min_nnz = 5 masks the thin bins; the hanger, whose every count is shared with one of
    them, has 5 non-zero cells but no count left among the live bins."""
    m, special = bm.integer_map(129, 129)
    a = bm.counted_cells(m)
    live0 = bm.balance_mask(a, 0)
    live5 = bm.balance_mask(a, 5)
    h, thin = special["hanger"], special["thin"]
    assert live0[h] and live0[thin].all()
    assert (a[h] != 0).sum() == 5 and not live5[h] and not live5[thin].any()
    assert live0[special["far"]] and not bm.balance_mask(bm.counted_cells(m, 65), 0)[special["far"]]


def test_model_exact_updates_and_band():
    """tol = 0, max_iter = K makes exactly K updates and K + 1 products; a NaN inside the ignored
    band is not counted, one outside is refused."""
    m = numpy.array(bm.hic_like_raw(66))
    r = bm.balance(m, tol=0.0, max_iter=7)
    assert r["iterations"] == 7 and len(r["variances"]) == 8 and not r["converged"]
    m[3, 4] = numpy.nan
    assert bm.offending_cells(m, 2) == 0 and bm.offending_cells(m, 1) == 1
    assert numpy.isfinite(bm.balance(m, ignore_diags=2)["variance"])
    with pytest.raises(ValueError):
        bm.balance(m, ignore_diags=1)


# ---- 3. the Hi-C-like generator stops clear of tol ---------------------------------------------------
@pytest.mark.parametrize("d,ignore_diags,min_nnz", bm.STOP_CASES)
def test_generator_stops_clear_of_tol(d, ignore_diags, min_nnz):
    """At the iteration where the model stops for tol = 1e-5, var is at least 1 % away from tol on
    both sides of the stop: rounding (1e-13 relative on var) cannot move the stop, so the device
    must make the same number of updates."""
    tol = 1e-5
    r = bm.hic_like_balance(d, ignore_diags, min_nnz, tol, 200)
    v = r["variances"]
    print("d=%d: stops after %d updates at var %.3e, the value before %.3e (ratio %.2f)"
          % (d, r["iterations"], v[-1], v[-2], v[-2] / v[-1]))
    assert r["converged"] and r["iterations"] >= 2
    assert v[-1] < 0.99 * tol and v[-2] > 1.01 * tol
