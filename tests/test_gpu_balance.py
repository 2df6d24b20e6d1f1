"""GPU: `ContactMap.balance` and `ContactMap.expected` (docs/SPEC.md 2.5.2) against the numpy
model of tests/_balance_model.py.

Sizes.  Both calls work on the leading n x n block, n = n_bins = d - 1, and both cut it as symv
cuts its matrix: row blocks of 64 and segments of 4,096 (columns for the product, diagonals for
the diagonal pass).  d = 2 is the one-bin map; 64, 65, 66 and 129 put n on and around a row-block
edge; 4,096 / 4,097 / 4,098 put n at 4,095 / 4,096 / 4,097, i.e. the last one-segment sizes and a
second segment one wide; 4,161 / 4,162 move a whole row block into the second segment; 8,193 fills
two segments.

  exact       integer maps: every partial sum is an integer below 2^53, so the diagonal sums,
              their counts and the mask must EQUAL the model's whatever the order of addition.
  toleranced  the Hi-C-like generator: after exactly 20 updates every live b_i is within
              (d + 16) 2^-52 relative of the model -- the worst case of ONE sum of d non-negative
              terms on each side; the iteration is contractive, so errors do not build up over
              the updates (two summation orders of the model differ by 1.6e-15 at d = 1,500, the model
              and its numpy.longdouble form by 8.9e-16, against a bound of 3.4e-13) --
              and e_k from the model's bias within the same bound.  The stopping rule: the same
              number of updates as the model (tests/test_balance_cpu.py asserts that the model
              stops at least 1 % clear of tol on both sides for these very cases).
  bits        the same bits on every run and after other calls have used the scratch; the matrix
              unchanged without `apply`; `apply` and `normalize()` are the existing normalize path.

Every toleranced figure is printed before it is asserted (`pytest -s`)."""
import numpy
import pytest

import blueberry_amd as bb
from blueberry_amd.datatypes import expected_from_sums
from tests import _balance_model as bm
from tests import _large_maps as lm
from tests._util import max_rel, same_bits

pytestmark = pytest.mark.gpu

SIZES = [2, 3, 64, 65, 66, 129, 4096, 4097, 4098, 4161, 4162, 8193]
# ignore_diags = 17: with 0 (the plain product's offsets) the one band at which a 64-column chunk
# starts exactly 15 + max(ignore_diags, 1) columns after a wave's first row -- the chunk at which
# the product's body chooses between its select branch and its plain one; one row block, and a
# whole row block in the second segment.  The model leaves 125 and 4,025 live bins of the
# Hi-C-like map under that band, 113 and 3,893 of the integer map at min_nnz = 5.
BAND17_SIZES = [129, 4161]
EPS = 2.0 ** -52


# ---- 1. exact: integer maps ----------------------------------------------------------------------
@pytest.mark.parametrize("d", SIZES)
def test_expected_sums_and_counts_equal_the_model_on_integer_maps(d):
    """bias=None: sum_k is the plain sum of diagonal k, cnt_k = n - k.  Then a 0/1 weight (bias 1
    or NaN): the pairs with a NaN end leave both.  Row and column n_bins hold NaN, -1 and inf."""
    m, special = bm.integer_map(d, d)
    n = d - 1
    cm = bb.ContactMap.from_matrix(m)
    e = cm.expected(bias=None)
    sums, counts, want = bm.expected(m, None)
    assert cm.expected_counts_.dtype == numpy.int64
    assert numpy.array_equal(cm.expected_counts_, counts) and numpy.array_equal(counts, n - numpy.arange(n))
    wrong = numpy.flatnonzero(cm.expected_sums_ != sums)
    assert wrong.size == 0, (d, wrong[:8], cm.expected_sums_[wrong[:8]], sums[wrong[:8]])
    assert same_bits(e, want) and e is cm._KRexpected
    assert same_bits(e, expected_from_sums(sums, counts))
    bias = numpy.ones(n)
    bias[numpy.random.default_rng(d).random(n) < 0.3] = numpy.nan
    e2 = cm.expected(bias=bias)
    sums2, counts2, want2 = bm.expected(m, bias)
    assert numpy.array_equal(cm.expected_counts_, counts2)
    assert numpy.array_equal(cm.expected_sums_, sums2)
    assert same_bits(e2, want2)
    assert same_bits(cm.to_host(), m)                             # nothing was written


def check_mask_equals_the_model(d, bands):
    m, special = bm.integer_map(d, d)
    cm = bb.ContactMap.from_matrix(m)
    seen_hanger = False
    for ignore_diags in bands:
        a = bm.counted_cells(m, ignore_diags)
        for min_nnz in (0, 5):
            live = bm.balance_mask(a, min_nnz)
            if not live.any():
                with pytest.raises(ValueError, match="no live bin"):
                    cm.balance(ignore_diags=ignore_diags, min_nnz=min_nnz, tol=0.0, max_iter=0)
                continue
            b = cm.balance(ignore_diags=ignore_diags, min_nnz=min_nnz, tol=0.0, max_iter=0)
            assert cm.balance_masked_.dtype == bool
            wrong = numpy.flatnonzero(cm.balance_masked_ != ~live)
            assert wrong.size == 0, (d, ignore_diags, min_nnz, wrong[:8])
            assert numpy.array_equal(numpy.isnan(b), ~live)
            assert numpy.array_equal(b[live], numpy.ones(int(live.sum())))   # no update was made
            assert cm.balance_iterations_ == 0
            if special and min_nnz == 5 and ignore_diags == 0:
                h = special["hanger"]
                seen_hanger = (a[h] != 0).sum() >= 5 and cm.balance_masked_[h]
    assert seen_hanger == (bool(special) and 0 in bands)      # (the hanger is looked for at band 0)
    assert same_bits(cm.to_host(), m)


@pytest.mark.parametrize("d", SIZES)
def test_mask_equals_the_model_on_integer_maps(d):
    """ignore_diags in {0, 1, 2, 65} x min_nnz in {0, 5}: dead rows, the thin bins (min_nnz), the
    hanger (the mask's fixed point) and the bin whose counts all lie inside a band of 65."""
    check_mask_equals_the_model(d, (0, 1, 2, 65))


@pytest.mark.parametrize("d", BAND17_SIZES)
def test_mask_equals_the_model_under_a_band_of_17(d):
    check_mask_equals_the_model(d, (17,))


def test_a_map_inside_the_ignored_band_masks_every_bin():
    n = 200
    m = numpy.zeros((n + 1, n + 1))
    i = numpy.arange(n)
    m[i, i] = 5.0
    m[i[:-1], i[:-1] + 1] = m[i[:-1] + 1, i[:-1]] = 3.0
    cm = bb.ContactMap.from_matrix(m)
    with pytest.raises(ValueError, match="no live bin"):
        cm.balance(ignore_diags=2)
    assert cm._KRnorm is None and same_bits(cm.to_host(), m)
    assert cm.balance(ignore_diags=1).shape == (n,)               # one diagonal less: it balances


def test_junk_in_row_and_column_n_bins_changes_nothing():
    d = 130
    clean = numpy.array(bm.hic_like_raw(d))
    junk = clean.copy()
    junk[d - 1, :] = numpy.tile([numpy.nan, -1.0, numpy.inf], d)[:d]
    junk[:, d - 1] = numpy.tile([-numpy.inf, 1e300, numpy.nan], d)[:d]
    out = []
    for m in (clean, junk):
        cm = bb.ContactMap.from_matrix(m)
        b = cm.balance(ignore_diags=1, min_nnz=3)
        e = cm.expected()
        out.append((b, e, cm.expected_sums_, cm.expected_counts_, cm.balance_iterations_))
        assert same_bits(cm.to_host(), m)
    assert same_bits(out[0][0], out[1][0]) and same_bits(out[0][1], out[1][1])
    assert same_bits(out[0][2], out[1][2]) and numpy.array_equal(out[0][3], out[1][3])
    assert out[0][4] == out[1][4]


# ---- 2. toleranced: the Hi-C-like generator ------------------------------------------------------
def check_twenty_updates_match_the_model(d, ignore_diags):
    want = bm.hic_like_balance(d, ignore_diags, 0, 0.0, 20)
    cm = bb.ContactMap.from_matrix(bm.hic_like_raw(d))
    if want is None:                                               # (d = 2, 3 under a band of 2)
        with pytest.raises(ValueError, match="no live bin"):
            cm.balance(ignore_diags=ignore_diags, tol=0.0, max_iter=20)
        return
    b = cm.balance(ignore_diags=ignore_diags, tol=0.0, max_iter=20)
    bound = (d + 16) * EPS
    err = max_rel(b, want["bias"])
    print("d=%d ignore_diags=%d: max relative error of b %.2e (bound %.2e), var %.3e (model %.3e), "
          "%d masked" % (d, ignore_diags, err, bound, cm.balance_variance_, want["variance"],
                         int(cm.balance_masked_.sum())))
    assert cm.balance_iterations_ == 20 and not cm.balance_converged_
    assert numpy.array_equal(cm.balance_masked_, want["masked"])
    assert err <= bound
    assert b is cm._KRnorm and b.dtype == numpy.float64 and b.shape == (d - 1,)


@pytest.mark.parametrize("ignore_diags", [0, 2])
@pytest.mark.parametrize("d", SIZES)
def test_twenty_updates_match_the_model(d, ignore_diags):
    check_twenty_updates_match_the_model(d, ignore_diags)


@pytest.mark.parametrize("d", BAND17_SIZES)
def test_twenty_updates_match_the_model_under_a_band_of_17(d):
    check_twenty_updates_match_the_model(d, 17)


@pytest.mark.parametrize("d", SIZES)
def test_expected_from_the_model_s_bias_matches_the_model(d):
    m = bm.hic_like_raw(d)
    model = bm.hic_like_balance(d, 0, 0, 0.0, 20)
    bias = numpy.full(d - 1, numpy.nan) if model is None else model["bias"]
    sums, counts, want = bm.expected(m, bias)
    cm = bb.ContactMap.from_matrix(m)
    e = cm.expected(bias=bias)
    bound = (d + 16) * EPS
    err = max_rel(e, want)
    print("d=%d: max relative error of e_k %.2e (bound %.2e), %d of %d diagonals without a value"
          % (d, err, bound, int(numpy.isnan(want).sum()), d - 1))
    assert numpy.array_equal(cm.expected_counts_, counts)
    assert err <= bound
    assert not (e == 0.0).any()


@pytest.mark.parametrize("d,ignore_diags,min_nnz", bm.STOP_CASES)
def test_stops_after_the_model_s_number_of_updates(d, ignore_diags, min_nnz):
    want = bm.hic_like_balance(d, ignore_diags, min_nnz, 1e-5, 200)
    cm = bb.ContactMap.from_matrix(bm.hic_like_raw(d))
    b = cm.balance(ignore_diags=ignore_diags, min_nnz=min_nnz, tol=1e-5)
    rel = abs(cm.balance_variance_ / want["variance"] - 1.0)
    print("d=%d: %d updates (model %d), var %.6e (model %.6e, relative difference %.2e)"
          % (d, cm.balance_iterations_, want["iterations"], cm.balance_variance_, want["variance"], rel))
    assert cm.balance_iterations_ == want["iterations"]
    assert cm.balance_converged_ is True
    assert rel < 1e-9
    assert numpy.array_equal(cm.balance_masked_, want["masked"])
    assert max_rel(b, want["bias"]) <= (d + 16) * EPS
    # row_sum = 1.0: the same vector on cooler's scale, sqrt(mean marginal) times larger
    b1 = cm.balance(ignore_diags=ignore_diags, min_nnz=min_nnz, tol=1e-5, row_sum=1.0)
    want1 = bm.balance(bm.hic_like_raw(d), ignore_diags, min_nnz, 1e-5, 200, row_sum=1.0)
    assert max_rel(b1, want1["bias"]) <= (d + 16) * EPS


@pytest.mark.parametrize("d", [129, 4097])
def test_exhausted_iterations_end_unconverged(d):
    cm = bb.ContactMap.from_matrix(bm.hic_like_raw(d))
    cm.balance(max_iter=3)
    want = bm.hic_like_balance(d, 0, 0, 1e-5, 3)
    print("d=%d: var after 3 updates %.6e (model %.6e)" % (d, cm.balance_variance_, want["variance"]))
    assert cm.balance_iterations_ == 3 and cm.balance_converged_ is False
    assert want["iterations"] == 3 and not want["converged"]
    assert abs(cm.balance_variance_ / want["variance"] - 1.0) < 1e-9


# ---- 3. bit for bit ------------------------------------------------------------------------------
def test_same_bits_on_every_run_and_after_other_calls_on_the_scratch():
    """Two runs, a run on a fresh map, and a run after the handle's partial-sum scratch has held
    the diagonal pass's sums, another band's products, and after a large correlation has been
    through the device's shared scratch: the same bits."""
    d = 4162
    m = bm.hic_like_raw(d)
    cm = bb.ContactMap.from_matrix(m)
    b1 = cm.balance(ignore_diags=2, min_nnz=10).copy()
    it1, var1 = cm.balance_iterations_, cm.balance_variance_
    e1 = cm.expected().copy()
    b2 = cm.balance(ignore_diags=2, min_nnz=10).copy()
    assert same_bits(b1, b2) and (it1, var1) == (cm.balance_iterations_, cm.balance_variance_)
    cm.balance(ignore_diags=0, tol=0.0, max_iter=2)
    big = bb.ContactMap.from_matrix(lm.cheap_symmetric(4500))
    big.correlation()
    del big
    b3 = cm.balance(ignore_diags=2, min_nnz=10).copy()
    e3 = cm.expected().copy()
    assert same_bits(b1, b3) and same_bits(e1, e3)
    fresh = bb.ContactMap.from_matrix(numpy.array(m))
    b4 = fresh.balance(ignore_diags=2, min_nnz=10)
    e4 = fresh.expected()
    assert same_bits(b1, b4) and same_bits(e1, e4)
    assert (it1, var1) == (fresh.balance_iterations_, fresh.balance_variance_)
    assert same_bits(cm.to_host(), m)                             # apply=False throughout


@pytest.mark.parametrize("d", [66, 300])
def test_apply_and_normalize_are_the_existing_normalize_path(d):
    m = numpy.array(bm.hic_like_raw(d))
    n = d - 1
    # balance(apply=True) = normalize() with (b, ones)
    cm = bb.ContactMap.from_matrix(m)
    b = cm.balance(ignore_diags=1, apply=True)
    ref = bb.ContactMap.from_matrix(m, KRnorm=b, KRexpected=numpy.ones(n))
    ref.normalize()
    got = cm.to_host()
    assert same_bits(got, ref.to_host())
    dead = numpy.flatnonzero(cm.balance_masked_)
    assert dead.size and not got[dead, :].any() and not got[:, dead].any()
    assert numpy.isnan(b[dead]).all()
    # balance(); expected(); normalize() = normalize() with the two returned vectors
    cm = bb.ContactMap.from_matrix(m)
    b = cm.balance(ignore_diags=1)
    e = cm.expected()
    assert same_bits(cm.to_host(), m)
    cm.normalize()
    ref = bb.ContactMap.from_matrix(m, KRnorm=b, KRexpected=e)
    ref.normalize()
    assert same_bits(cm.to_host(), ref.to_host())
    assert numpy.isfinite(cm.to_host()).all()
    # expected(apply=True) divides by e alone
    cm = bb.ContactMap.from_matrix(m)
    e0 = cm.expected(bias=None, apply=True)
    ref = bb.ContactMap.from_matrix(m, KRnorm=numpy.ones(n), KRexpected=e0)
    ref.normalize()
    assert same_bits(cm.to_host(), ref.to_host())
    # filter() drops what describes the unfiltered map
    cm.filter(0)
    assert cm._KRnorm is None and cm._KRexpected is None
    assert cm.balance_masked_ is None and cm.expected_sums_ is None and cm.expected_counts_ is None
    with pytest.raises(ValueError):
        cm.normalize()


# ---- 4. refusals ---------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [-1.0, numpy.nan, numpy.inf])
def test_bad_entries_are_refused_and_the_map_is_left_alone(value):
    d = 4100
    base = bm.hic_like_raw(d)
    for (i, j), ignore_diags, counted in (((7, 7), 0, True),          # on the diagonal
                                          ((70, 4099 - 1), 0, True),   # second column segment
                                          ((3000, 3001), 2, False),    # inside the ignored band
                                          ((3000, 3002), 2, True)):
        m = numpy.array(base)
        m[i, j] = value                     # the upper triangle is what is read
        m[j, i] = value
        cm = bb.ContactMap.from_matrix(m)
        if counted:
            with pytest.raises(ValueError, match="1 counted cells") as err:
                cm.balance(ignore_diags=ignore_diags)
            assert "negative or not finite" in str(err.value)
            assert cm._KRnorm is None
        else:
            b = cm.balance(ignore_diags=ignore_diags)
            assert numpy.isfinite(b[~cm.balance_masked_]).all() and cm.balance_converged_
        assert same_bits(cm.to_host(), m)
    m = numpy.array(base)
    m[5, 900] = m[900, 5] = value
    m[64, 64] = value
    m[4000, 4098] = m[4098, 4000] = value
    cm = bb.ContactMap.from_matrix(m)
    with pytest.raises(ValueError, match="3 counted cells"):
        cm.balance()
    assert same_bits(cm.to_host(), m)
