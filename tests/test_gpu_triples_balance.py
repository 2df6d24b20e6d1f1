"""GPU: balancing straight from triples -- `balance_triples`, `DeviceTriples.balance` /
`.expected`, `StructureSolver.fit_triples(balance=...)` (docs/SPEC.md 2.5.3) -- against the dense
model of tests/_balance_model.py on the same maps given as triples, against the sparse model of
tests/_triples_model.py where no dense matrix can be made, and against the dense device path.

  exact       integer maps: the mask, the expected's sums and counts, the number of stored pairs.
  toleranced  after exactly 20 updates every live b_i within (d + 16) 2^-52 relative of the model,
              d = n_bins + 1: the bound of tests/test_gpu_balance.py -- ONE sum of at most d
              non-negative terms on each side, the iteration contractive -- and e_k from the
              model's bias within the same bound.  At n_bins = 70,000 (keys above 2^32) two
              summation orders of the float64 model and its longdouble form differ by 1.4e-15
              after 20 updates under a band of 2, against a bound of 1.6e-11.
  bits        the same bits on every run, from a fresh handle, after a fit has used the handle,
              and for every duplicate-free list of the same pairs.
The product gives a wave a segment of SEG entries of one row; row shapes are chosen around it.
Every toleranced figure is printed before it is asserted (`pytest -s`)."""
import ctypes

import numpy
import pytest

import blueberry_amd as bb
from blueberry_amd import _lib
from tests import _balance_model as bm
from tests import _triples_model as tm
from tests._util import max_rel, same_bits

pytestmark = pytest.mark.gpu

SIZES = [2, 3, 64, 65, 66, 129, 4097]
BAND17_SIZES = [129, 4097]
EPS = 2.0 ** -52
RES = tm.RESOLUTION
SEG = 1024          # kTbSeg of bb_triples_balance.hip: the entries of a row one wave sums


_lists = {}


def hic_list(d):
    """The Hi-C-like dense map of edge d as triples, made once.  READ-ONLY."""
    if ("hic", d) not in _lists:
        _lists["hic", d] = tm.triples_of_matrix(bm.hic_like_raw(d))
    return _lists["hic", d]


def integer_list(d):
    """(triples, matrix) of the integer map of edge d (its junk border included as triples that
    touch bin n_bins), made once.  READ-ONLY."""
    if ("int", d) not in _lists:
        m = bm.integer_map(d, d)[0]
        _lists["int", d] = (tm.triples_of_matrix(m), m)
    return _lists["int", d]


# ---- 1. against the dense model --------------------------------------------------------------
def check_mask(d, bands):
    t, m = integer_list(d)
    n = d - 1
    dev = bb.DeviceTriples(t, RES, 0)
    for ignore_diags in bands:
        a = bm.counted_cells(m, ignore_diags)
        for min_nnz in (0, 5):
            live = bm.balance_mask(a, min_nnz)
            if not live.any():
                with pytest.raises(ValueError, match="no live bin"):
                    dev.balance(n, ignore_diags=ignore_diags, min_nnz=min_nnz, tol=0.0, max_iter=0)
                continue
            b = dev.balance(n, ignore_diags=ignore_diags, min_nnz=min_nnz, tol=0.0, max_iter=0)
            assert dev.balance_masked_.dtype == bool
            wrong = numpy.flatnonzero(dev.balance_masked_ != ~live)
            assert wrong.size == 0, (d, ignore_diags, min_nnz, wrong[:8])
            assert numpy.array_equal(numpy.isnan(b), ~live)
            assert numpy.array_equal(b[live], numpy.ones(int(live.sum())))
            assert dev.balance_iterations_ == 0
    dev.close()


@pytest.mark.parametrize("d", SIZES)
def test_mask_equals_the_model_on_integer_maps(d):
    check_mask(d, (0, 1, 2, 65))


@pytest.mark.parametrize("d", BAND17_SIZES)
def test_mask_equals_the_model_under_a_band_of_17(d):
    check_mask(d, (17,))


def check_twenty_updates(d, ignore_diags):
    want = bm.hic_like_balance(d, ignore_diags, 0, 0.0, 20)
    if want is None:
        with pytest.raises(ValueError, match="no live bin"):
            bb.balance_triples(hic_list(d), RES, d - 1, ignore_diags=ignore_diags, tol=0.0, max_iter=20)
        return
    r = bb.balance_triples(hic_list(d), RES, d - 1, ignore_diags=ignore_diags, tol=0.0, max_iter=20)
    bound = (d + 16) * EPS
    err = max_rel(r.bias, want["bias"])
    print("d=%d ignore_diags=%d: max relative error of b %.2e (bound %.2e), var %.3e (model %.3e), "
          "%d masked" % (d, ignore_diags, err, bound, r.variance, want["variance"], int(r.masked.sum())))
    assert r.iterations == 20 and not r.converged
    assert numpy.array_equal(r.masked, want["masked"])
    assert err <= bound
    assert r.bias.dtype == numpy.float64 and r.bias.shape == (d - 1,) and r.expected is None


@pytest.mark.parametrize("ignore_diags", [0, 2])
@pytest.mark.parametrize("d", SIZES)
def test_twenty_updates_match_the_model(d, ignore_diags):
    check_twenty_updates(d, ignore_diags)


@pytest.mark.parametrize("d", BAND17_SIZES)
def test_twenty_updates_match_the_model_under_a_band_of_17(d):
    check_twenty_updates(d, 17)


@pytest.mark.parametrize("d,ignore_diags,min_nnz", [c for c in bm.STOP_CASES if c[0] <= 4097])
def test_stops_after_the_model_s_number_of_updates(d, ignore_diags, min_nnz):
    want = bm.hic_like_balance(d, ignore_diags, min_nnz, 1e-5, 200)
    dev = bb.DeviceTriples(hic_list(d), RES, 0)
    b = dev.balance(d - 1, ignore_diags=ignore_diags, min_nnz=min_nnz, tol=1e-5)
    rel = abs(dev.balance_variance_ / want["variance"] - 1.0)
    print("d=%d: %d updates (model %d), var %.6e (model %.6e, relative difference %.2e)"
          % (d, dev.balance_iterations_, want["iterations"], dev.balance_variance_, want["variance"], rel))
    assert dev.balance_iterations_ == want["iterations"]
    assert dev.balance_converged_ is True
    assert rel < 1e-9
    assert numpy.array_equal(dev.balance_masked_, want["masked"])
    assert max_rel(b, want["bias"]) <= (d + 16) * EPS
    b1 = dev.balance(d - 1, ignore_diags=ignore_diags, min_nnz=min_nnz, tol=1e-5, row_sum=1.0)
    want1 = bm.balance(bm.hic_like_raw(d), ignore_diags, min_nnz, 1e-5, 200, row_sum=1.0)
    err1 = max_rel(b1, want1["bias"])
    print("   row_sum=1.0: max relative error of b %.2e" % err1)
    assert err1 <= (d + 16) * EPS
    dev.close()


@pytest.mark.parametrize("d", [129, 4097])
def test_exhausted_iterations_end_unconverged(d):
    r = bb.balance_triples(hic_list(d), RES, d - 1, max_iter=3)
    want = bm.hic_like_balance(d, 0, 0, 1e-5, 3)
    print("d=%d: var after 3 updates %.6e (model %.6e)" % (d, r.variance, want["variance"]))
    assert r.iterations == 3 and r.converged is False
    assert want["iterations"] == 3 and not want["converged"]
    assert abs(r.variance / want["variance"] - 1.0) < 1e-9


@pytest.mark.parametrize("d", SIZES)
def test_expected_sums_and_counts_equal_the_model_on_integer_maps(d):
    """bias=None, then a bias of powers of two with NaN at 30 % of the bins: every product and
    every partial sum is exact, so sums and counts must EQUAL the dense model's."""
    t, m = integer_list(d)
    n = d - 1
    dev = bb.DeviceTriples(t, RES, 0)
    e = dev.expected(n)
    sums, counts, want = bm.expected(m, None)
    assert dev.expected_counts_.dtype == numpy.int64
    assert numpy.array_equal(dev.expected_counts_, counts) and numpy.array_equal(counts, n - numpy.arange(n))
    wrong = numpy.flatnonzero(dev.expected_sums_ != sums)
    assert wrong.size == 0, (d, wrong[:8], dev.expected_sums_[wrong[:8]], sums[wrong[:8]])
    assert same_bits(e, want)
    rng = numpy.random.default_rng(d)
    bias = 2.0 ** rng.integers(-3, 4, size=n)
    bias[rng.random(n) < 0.3] = numpy.nan
    e2 = dev.expected(n, bias)
    sums2, counts2, want2 = bm.expected(m, bias)
    assert numpy.array_equal(dev.expected_counts_, counts2)
    assert numpy.array_equal(dev.expected_sums_, sums2)
    assert same_bits(e2, want2)
    dev.close()


@pytest.mark.parametrize("d", SIZES)
def test_expected_from_the_model_s_bias_matches_the_model(d):
    m = bm.hic_like_raw(d)
    model = bm.hic_like_balance(d, 0, 0, 0.0, 20)
    bias = numpy.full(d - 1, numpy.nan) if model is None else model["bias"]
    sums, counts, want = bm.expected(m, bias)
    dev = bb.DeviceTriples(hic_list(d), RES, 0)
    e = dev.expected(d - 1, bias)
    bound = (d + 16) * EPS
    err = max_rel(e, want)
    print("d=%d: max relative error of e_k %.2e (bound %.2e), %d of %d diagonals without a value"
          % (d, err, bound, int(numpy.isnan(want).sum()), d - 1))
    assert numpy.array_equal(dev.expected_counts_, counts)
    assert err <= bound
    assert not (e == 0.0).any()
    dev.close()


# ---- 2. against the sparse model: keys above 2^32 ----------------------------------------------
BIG = 70000
# the model's var is 5.6023e-3 after 11 updates and 5.4095e-3 after 12: tol is clear of both
BIG_TOL = 5.5e-3


def test_seventy_thousand_bins_match_the_sparse_model():
    n = BIG
    assert n * n > 2 ** 32
    t = tm.hic_like_triples(n)
    bound = (n + 1 + 16) * EPS
    dev = bb.DeviceTriples(t, RES, 0)
    want = tm.hic_like_triples_balance(n, 2, 0, 0.0, 20)
    b = dev.balance(n, ignore_diags=2, tol=0.0, max_iter=20)
    err = max_rel(b, want["bias"])
    print("n_bins=%d, %d pairs: max relative error of b %.2e (bound %.2e), %d masked"
          % (n, t.shape[0], err, bound, int(dev.balance_masked_.sum())))
    assert dev.pairs(n) == t.shape[0]
    assert dev.balance_iterations_ == 20 and numpy.array_equal(dev.balance_masked_, want["masked"])
    assert err <= bound
    # the stopping rule
    stop = tm.hic_like_triples_balance(n, 2, 0, BIG_TOL, 200)
    v = stop["variances"]
    assert v[-1] < 0.99 * BIG_TOL and v[-2] > 1.01 * BIG_TOL       # (the model stops clear of tol)
    b2 = dev.balance(n, ignore_diags=2, tol=BIG_TOL)
    rel = abs(dev.balance_variance_ / stop["variance"] - 1.0)
    print("   %d updates (model %d), var relative difference %.2e"
          % (dev.balance_iterations_, stop["iterations"], rel))
    assert dev.balance_iterations_ == stop["iterations"] and dev.balance_converged_ is True
    assert rel < 1e-9 and max_rel(b2, stop["bias"]) <= bound
    # the expected: counts of ALL k equal, e within the bound and never 0
    sums, counts, e_want = tm.expected(t, RES, n, want["bias"])
    e = dev.expected(n, want["bias"])
    err = max_rel(e, e_want)
    print("   max relative error of e_k %.2e, %d diagonals with a value" % (err, int((~numpy.isnan(e)).sum())))
    assert numpy.array_equal(dev.expected_counts_, counts)
    assert err <= bound and not (e == 0.0).any()
    e0 = dev.expected(n)
    s0, c0, _ = tm.expected(t, RES, n, None)
    assert numpy.array_equal(dev.expected_counts_, c0) and numpy.array_equal(dev.expected_sums_, s0)
    dev.close()


# ---- 3. the same on the dense device path ------------------------------------------------------
@pytest.mark.parametrize("d", [66, 129, 4097])
def test_the_dense_device_path_agrees(d):
    n = d - 1
    t = hic_list(d)
    cm = bb.ContactMap.from_triples(t, RES, n)
    r = bb.balance_triples(t, RES, n, ignore_diags=2, min_nnz=10, expected=True)
    b = cm.balance(ignore_diags=2, min_nnz=10)
    e = cm.expected()
    bound = (d + 16) * EPS
    err, err_e = max_rel(r.bias, b), max_rel(r.expected, e)      # (e: each side from its own bias)
    print("d=%d: triples against the dense device path: b %.2e (bound %.2e), e %.2e" % (d, err, bound, err_e))
    assert numpy.array_equal(r.masked, cm.balance_masked_)
    assert r.iterations == cm.balance_iterations_ and r.converged == cm.balance_converged_
    assert numpy.array_equal(r.expected_counts, cm.expected_counts_)
    assert err <= bound


# ---- 4. the index ------------------------------------------------------------------------------
def integer_pairs(n, count, rng, diagonal=0):
    """`count` distinct pairs i < j < n and `diagonal` pairs i == i, integer counts, shuffled."""
    key = numpy.unique(rng.integers(0, n, size=3 * count) * n + rng.integers(0, n, size=3 * count))
    key = rng.permutation(key[key // n < key % n])[:count]
    assert key.shape[0] == count
    i, j = key // n, key % n
    dg = rng.choice(n, size=diagonal, replace=False)
    i, j = numpy.concatenate([i, dg]), numpy.concatenate([j, dg])
    order = rng.permutation(i.shape[0])
    c = rng.integers(1, 1000, size=i.shape[0]).astype(numpy.float64)
    return numpy.column_stack([i[order] * float(RES), j[order] * float(RES), c])


def test_the_last_triple_of_a_pair_wins():
    n = 4096
    rng = numpy.random.default_rng(1)
    t = integer_pairs(n, 299000, rng, diagonal=1000)
    assert t.shape[0] == 300000
    i, j = (t[:, 0] / RES).astype(int), (t[:, 1] / RES).astype(int)
    # a pair the list does not hold yet takes over three rows, in both orientations
    a, b = 1234, 2345
    t = t[~(((i == a) & (j == b)) | ((i == b) & (j == a)))][:300000]
    for at, (p, q, c) in ((5, (a, b, 11.0)), (150000, (b, a, 22.0)), (299990, (a, b, 33.0))):
        t[at] = [p * RES, q * RES, c]
    dev = bb.DeviceTriples(t, RES, 0)
    ui, uj, uv = tm.upper_cells(t, RES, n)
    assert dev.pairs(n) == ui.shape[0] and (ui == uj).sum() >= 990       # a diagonal triple: one pair
    dev.expected(n)
    sums, counts, _ = tm.expected(t, RES, n, None)
    assert numpy.array_equal(dev.expected_sums_, sums) and numpy.array_equal(dev.expected_counts_, counts)
    # ... and sums[b - a] holds 33, neither 11 nor 22
    other = t.copy()
    other[299990, 2] = 34.0
    d2 = bb.DeviceTriples(other, RES, 0)
    d2.expected(n)
    diff = d2.expected_sums_ - dev.expected_sums_
    assert diff[b - a] == 1.0 and numpy.count_nonzero(diff) == 1
    dev.close()
    d2.close()


def test_a_pair_that_touches_bin_n_bins_changes_nothing_and_bad_bins_are_refused():
    d = 130
    n = d - 1
    t = tm.triples_of_matrix(bm.hic_like_raw(d), border=False)
    plain = bb.balance_triples(t, RES, n, ignore_diags=1, expected=True)
    border = numpy.array([[n * RES, 3 * RES, numpy.nan], [5 * RES, n * RES + 1, -1.0],
                          [n * RES, n * RES, numpy.inf]])
    both = bb.balance_triples(numpy.concatenate([border, t, border]), RES, n, ignore_diags=1, expected=True)
    assert same_bits(plain.bias, both.bias) and same_bits(plain.expected_sums, both.expected_sums)
    assert numpy.array_equal(plain.expected_counts, both.expected_counts)
    # a bin of n_bins + 1, a negative position: refused as the scatter refuses them, nothing
    # half-built -- the next call on the same handle (one bin more makes the first legal) succeeds
    for bad in ([(n + 1) * RES, 0.0, 1.0], [0.0, -2.0 * RES, 1.0], [numpy.inf, 0.0, 1.0]):
        dev = bb.DeviceTriples(numpy.concatenate([t, [bad]]), RES, 0)
        for call in (lambda: dev.balance(n), lambda: dev.expected(n), lambda: dev.pairs(n)):
            with pytest.raises(ValueError, match=r"a position maps to a bin outside \[0, n_bins\]"):
                call()
        with pytest.raises(ValueError, match=r"outside \[0, n_bins\]"):
            bb.ContactMap.from_triples(numpy.concatenate([t, [bad]]), RES, n)
        if bad[0] == (n + 1) * RES:
            first = dev.balance(n + 1, ignore_diags=1)
            with pytest.raises(ValueError, match="outside"):
                dev.balance(n, ignore_diags=1)
            assert same_bits(first, dev.balance(n + 1, ignore_diags=1))
            assert same_bits(first[:n], plain.bias) and numpy.isnan(first[n])
        dev.close()


def test_the_input_check():
    d = 130
    n = d - 1
    t = tm.triples_of_matrix(bm.hic_like_raw(d), border=False)
    i, j = (t[:, 0] / RES).astype(int), (t[:, 1] / RES).astype(int)
    # a bin r whose cells (r, r + 1) and (r, r + 3) are both stored
    cells = set(zip(i.tolist(), j.tolist()))
    r = next(r for r in range(20, n - 3) if (r, r + 1) in cells and (r, r + 3) in cells)
    at = int(numpy.flatnonzero((i == r) & (j == r + 1))[0])
    far = int(numpy.flatnonzero((i == r) & (j == r + 3))[0])
    # a NaN count is a zero cell
    nan, zero = t.copy(), t.copy()
    nan[far, 2], zero[far, 2] = numpy.nan, 0.0
    assert same_bits(bb.balance_triples(nan, RES, n).bias, bb.balance_triples(zero, RES, n).bias)
    neg = t.copy()
    neg[at, 2] = -1.0
    with pytest.raises(ValueError, match="1 counted cells") as err:
        bb.balance_triples(neg, RES, n, ignore_diags=1)
    assert "negative" in str(err.value)
    r = bb.balance_triples(neg, RES, n, ignore_diags=2)           # inside the ignored band
    assert numpy.isfinite(r.bias[~r.masked]).all() and r.converged
    neg[far, 2] = -3.0
    neg = numpy.concatenate([neg, [[7 * RES, 7 * RES, -2.0]]])    # the diagonal cell, last wins
    with pytest.raises(ValueError, match="3 counted cells"):
        bb.balance_triples(neg, RES, n)
    with pytest.raises(ValueError, match="no live bin"):
        bb.balance_triples(numpy.zeros((0, 3)), RES, n)
    empty = bb.DeviceTriples(numpy.zeros((0, 3)), RES, 0)
    assert empty.pairs(n) == 0
    empty.expected(n)
    assert not empty.expected_sums_.any() and numpy.array_equal(empty.expected_counts_, n - numpy.arange(n))
    empty.close()


# ---- 5. row shapes ---------------------------------------------------------------------------
def row_shape_list():
    """n_bins = 8,192: the Hi-C-like list over the bins below 8,000, and above them bins whose rows
    hold exactly 0, 1, 63, 64 and 65 entries, a hub of 4 SEG + 37 entries, and a bin u whose only
    partners z1, z2 have one non-zero cell each (u itself)."""
    n = 8192
    base = numpy.array(tm.hic_like_triples(n))
    bi, bj = (base[:, 0] / RES).astype(int), (base[:, 1] / RES).astype(int)
    base = base[(bi < 8000) & (bj < 8000)]
    rng = numpy.random.default_rng(8192)
    special = {"empty": 8001, "one": 8002, "r63": 8003, "r64": 8004, "r65": 8005, "hub": 8006,
               "u": 8010, "z1": 8011, "z2": 8012}
    rows = []
    for name, first, count in (("one", 10, 1), ("r63", 100, 63), ("r64", 200, 64), ("r65", 300, 65),
                               ("hub", 0, 4 * SEG + 37)):
        p = numpy.arange(first, first + count)
        rows.append(numpy.column_stack([numpy.full(count, special[name] * float(RES)), p * float(RES),
                                        rng.integers(1, 50, size=count).astype(numpy.float64)]))
    rows.append(numpy.array([[special["u"] * RES, special["z1"] * RES, 4.0],
                             [special["z2"] * RES, special["u"] * RES, 9.0]]))
    return n, numpy.concatenate([base] + rows), special


def test_row_shapes_around_the_segment_length():
    n, t, special = row_shape_list()
    i, j, v = tm.upper_cells(t, RES, n)
    lengths = numpy.diff(tm.symmetric_csr(i, j, v, n).indptr)
    assert [int(lengths[special[k]]) for k in ("empty", "one", "r63", "r64", "r65", "hub")] == \
        [0, 1, 63, 64, 65, 4 * SEG + 37]
    bound = (n + 1 + 16) * EPS
    dev = bb.DeviceTriples(t, RES, 0)
    want = tm.balance(t, RES, n, 0, 0, 0.0, 20)
    b = dev.balance(n, tol=0.0, max_iter=20)
    err = max_rel(b, want["bias"])
    print("row shapes: max relative error of b %.2e (bound %.2e)" % (err, bound))
    assert numpy.array_equal(dev.balance_masked_, want["masked"]) and err <= bound
    assert dev.balance_masked_[special["empty"]] and not dev.balance_masked_[special["hub"]]
    for k in ("one", "r63", "r64", "r65", "u", "z1", "z2"):
        assert not dev.balance_masked_[special[k]]
    # min_nnz = 2 masks z1 and z2 (one non-zero cell each); u has two and passes, but its only
    # partners are masked: the fixed point masks it
    want = tm.balance(t, RES, n, 0, 2, 0.0, 20)
    b = dev.balance(n, min_nnz=2, tol=0.0, max_iter=20)
    assert lengths[special["u"]] == 2
    assert numpy.array_equal(dev.balance_masked_, want["masked"])
    assert all(dev.balance_masked_[special[k]] for k in ("u", "z1", "z2", "one"))
    assert max_rel(b, want["bias"]) <= bound
    dev.close()


# ---- 6. the word edges of the count kernel -----------------------------------------------------
@pytest.mark.parametrize("n", [63, 64, 65, 128, 129])
def test_pair_counts_at_the_word_edges(n):
    dead = sorted({b for b in (0, 63, 64, n - 1) if b < n})
    rng = numpy.random.default_rng(n)
    i = numpy.repeat(numpy.arange(n), 4)
    j = i + numpy.tile(numpy.arange(4), n)
    ok = j < n
    t = numpy.column_stack([i[ok] * float(RES), j[ok] * float(RES),
                            rng.integers(1, 100, size=int(ok.sum())).astype(numpy.float64)])
    bias = numpy.ones(n)
    bias[dead] = numpy.nan
    live = ~numpy.isnan(bias)
    brute = numpy.array([int((live[:n - k] & live[k:]).sum()) for k in range(n)])
    dev = bb.DeviceTriples(t, RES, 0)
    dev.expected(n, bias)
    sums, counts, _ = tm.expected(t, RES, n, bias)
    assert numpy.array_equal(counts, brute)
    assert numpy.array_equal(dev.expected_counts_, brute) and numpy.array_equal(dev.expected_sums_, sums)
    dev.expected(n)
    assert numpy.array_equal(dev.expected_counts_, n - numpy.arange(n))
    dev.close()


# ---- 7. bits -----------------------------------------------------------------------------------
def test_same_bits_on_every_run_from_every_list_of_the_same_pairs():
    n = 8192
    t = numpy.array(tm.hic_like_triples(n))
    kw = dict(ignore_diags=2, min_nnz=3, tol=0.0, max_iter=8)
    dev = bb.DeviceTriples(t, RES, 0)
    b1 = dev.balance(n, **kw)
    e1 = dev.expected(n, b1)
    s1 = dev.expected_sums_
    assert same_bits(b1, dev.balance(n, **kw)) and same_bits(e1, dev.expected(n, b1))     # again
    # ... after a fit has packed from the same handle
    bb.StructureSolver(n_iter=2, init="random").fit_triples(dev, RES, n)
    assert same_bits(b1, dev.balance(n, **kw)) and same_bits(s1, (dev.expected(n, b1), dev.expected_sums_)[1])
    dev.close()
    rng = numpy.random.default_rng(7)
    flipped = t[:, [1, 0, 2]]
    variants = {"fresh": t, "permuted": t[rng.permutation(t.shape[0])],
                "flipped": numpy.ascontiguousarray(flipped),
                "half flipped": numpy.where((rng.random(t.shape[0]) < 0.5)[:, None], flipped, t),
                "column-major": numpy.asfortranarray(t)}
    assert variants["column-major"].flags.f_contiguous and not variants["column-major"].flags.c_contiguous
    for name, v in variants.items():
        r = bb.balance_triples(v, RES, n, expected=True, **kw)
        assert same_bits(b1, r.bias), name
        assert same_bits(s1, r.expected_sums) and same_bits(e1, r.expected), name


def test_fit_triples_balance_is_fit_triples_with_the_bias():
    d = 130
    n = d - 1
    t = tm.triples_of_matrix(bm.hic_like_raw(d), border=False)
    r = bb.balance_triples(t, RES, n, ignore_diags=2, expected=True)
    for expected in (False, True):
        ke = r.expected if expected else numpy.ones(n)
        ref = bb.StructureSolver(n_iter=20, seed=3).fit_triples(t, RES, n, KRnorm=r.bias, KRexpected=ke)
        got = bb.StructureSolver(n_iter=20, seed=3).fit_triples(
            t, RES, n, balance=dict(ignore_diags=2, expected=expected))
        assert same_bits(got.structure_, ref.structure_) and same_bits(got.stress_, ref.stress_)
        assert same_bits(got.bias_, r.bias) and numpy.array_equal(got.balance_masked_, r.masked)
        assert got.balance_iterations_ == r.iterations and got.balance_converged_ == r.converged
        assert same_bits(got.expected_, r.expected) if expected else not hasattr(got, "expected_")
        assert numpy.isfinite(got.structure_).all() and got.stress_[-1] < got.stress_[0]
    with pytest.raises(ValueError, match="KRnorm"):
        bb.StructureSolver().fit_triples(t, RES, n, balance=True, KRnorm=r.bias, KRexpected=numpy.ones(n))
    # complete='shortest_path' balances the dense map through ContactMap.balance
    s = bb.StructureSolver(n_iter=5, seed=3).fit_triples(t, RES, n, balance=dict(ignore_diags=2),
                                                         complete="shortest_path")
    cm = bb.ContactMap.from_triples(t, RES, n)
    assert same_bits(s.bias_, cm.balance(ignore_diags=2)) and numpy.isfinite(s.structure_).all()


# ---- 8. lifetimes ------------------------------------------------------------------------------
def free_device_memory():
    hip = ctypes.CDLL([p for p in _lib.hip_runtimes_loaded() if "libamdhip64" in p][0])
    free, total = ctypes.c_size_t(), ctypes.c_size_t()
    assert hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
    return free.value


def test_fifty_handles_give_their_memory_back():
    """Create, balance, expected, destroy, 50 times: the device's free memory is back where it was
    after the first round.  The slack is one handle's triples (4.8 MB): a handle that kept its
    index, or its triples, would cost 50 times that or more."""
    n = 4096
    t = integer_pairs(n, 200000, numpy.random.default_rng(5))

    def once():
        dev = bb.DeviceTriples(t, RES, 0)
        dev.balance(n, tol=0.0, max_iter=2)
        dev.expected(n)
        dev.close()
    once()
    before = free_device_memory()
    for _ in range(50):
        once()
    after = free_device_memory()
    print("free device memory: %d before, %d after 50 handles" % (before, after))
    assert before - after <= t.nbytes
