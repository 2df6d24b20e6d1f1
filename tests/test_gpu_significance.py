"""GPU: `binomial_sf`, `FitHiC` and the two device routes behind it (docs/SPEC.md 2.9) against the
numpy model of tests/_fithic_model.py and the multi-precision truth of
tests/golden/binomial_sf_truth.npz.

Sizes.  Every kernel of bb_significance.hip runs workgroups of 256 threads = 4 waves.
`binomial_sf` gives an element to a thread: the lengths 0, 1, 63, 64, 65 (a wave), 255, 256, 257 (a
workgroup; 257 needs a second one) and 600.  The dense route gives a wave up to 1,024 columns of
one row's in-range span, so a row has ceil(span / 1,024) work items: d = n_bins + 1 in 2, 3, 65, 66,
129, and 1,025 / 1,026 / 1,027, where with the full range (k = 1 .. n - 1) row 0's span is 1,023,
1,024 (the last one-item size) and 1,025 (a second item one column wide).  The triples route cuts
the entries a row has in the canonical index (both directions of every stored pair) into segments
of 1,024; the rows of those maps stay below 500 entries, so `fm.long_rows_map` has rows of exactly
1,023, 1,024 and 1,025 entries (the last one-segment size and the first two past it) and one of
2,100 (three segments); its dense form has three items per row.

Tolerances.  p against the TRUTH: the model's measured worst, 1.64e-13, x 4 is the model's bound
(tests/test_fithic_cpu.py), and x 4 again, 2.62e-12, the device's: its exp / log / log1p are another
implementation.  p against the model under the same prior: that same 2.62e-12.  Everything else --
rows, columns, counts, N, T, the list's length, q from the device's own p -- is exact.

Measured on an MI355X (docs/MEASUREMENTS.md): the truth table within 1.19e-13 (row 344: k =
1,056,767, n = 3e9, p = 3.5e-4); the lists' p within 4.3e-14 of the model under the same prior.

Every toleranced figure is printed before it is asserted (`pytest -s`)."""
import ctypes

import numpy
import pytest

import blueberry_amd as bb
from blueberry_amd import _lib
from blueberry_amd import fithic as fh
from tests import _fithic_model as fm
from tests._util import same_bits

pytestmark = pytest.mark.gpu

RES = 10
DEVICE_BOUND = 16 * fm.MODEL_WORST
DENSE_SIZES = [2, 3, 65, 66, 129, 1025, 1026, 1027]
FULL = (0, 10000000)


def rel_to(got, want):
    """max |got / want - 1| over want >= 1e-290; below it got must be <= 1e-289."""
    got, want = numpy.asarray(got), numpy.asarray(want)
    big = want >= fm.TINY_TRUTH
    assert numpy.all((got[~big] >= 0) & (got[~big] <= fm.TINY_RESULT))
    return float(numpy.max(numpy.abs(got[big] / want[big] - 1.0))) if big.any() else 0.0


def ranges(n):
    """(min_dist, max_dist) of the cases of an n-bin map at RES: one diagonal, the full range."""
    if n == 1:
        return [(-1, 0)]                           # the one cell there is: k = 0
    return [(0, RES), FULL] if n > 2 else [FULL]


def device_list(X, n, min_dist, max_dist, bias, bias_range, prior, n_reads):
    """The device pass alone, below `FitHiC` (whose binning needs more bins than the smallest maps
    have): (row, col, count, p)."""
    ks = fm.in_range(n, RES, min_dist, max_dist)
    res = fh.significance_list(X, n, ks[0], ks[-1], numpy.ascontiguousarray(bias, dtype=numpy.float64),
                               bias_range, numpy.ascontiguousarray(prior, dtype=numpy.float64), n_reads)
    try:
        return res.read()
    finally:
        res.close()


def dense_case(d):
    """(n, the (n + 1)^2 map, the bias vector) of edge d; seed d, except 4 for the two-bin map,
    whose one off-diagonal cell seed 3 leaves empty."""
    n = d - 1
    m = fm.random_map(n, 4 if d == 3 else d)
    return n, m, fm.random_bias(n, d)


# ---- 1. binomial_sf --------------------------------------------------------------------------------
@pytest.mark.parametrize("length", [0, 1, 63, 64, 65, 255, 256, 257, 600])
def test_binomial_sf_lengths(length):
    rng = numpy.random.default_rng(length)
    k = rng.integers(-1, 40, length)
    p = rng.random(length) * 0.03
    if length > 2:
        p[0], p[1] = 0.0, 1.0
    got = bb.binomial_sf(k, 1000, p)
    want = fm.binomial_sf(k, 1000, p) if length else numpy.zeros(0)
    assert got.shape == (length,) and got.dtype == numpy.float64
    err = rel_to(got, want)
    print("length %d: max relative difference to the model %.3e (bound %.3e)" % (length, err, DEVICE_BOUND))
    assert err <= DEVICE_BOUND
    closed = (k <= 0) | (p == 0) | (p == 1)
    assert numpy.array_equal(got[closed], want[closed])


def table_on_device():
    t = fm.truth_table()
    got = numpy.empty(t["k"].shape[0])
    for n in numpy.unique(t["n"]):
        rows = t["n"] == n
        got[rows] = bb.binomial_sf(t["k"][rows], n, t["p"][rows])
    return got


def test_binomial_sf_against_the_truth_table():
    got = table_on_device()
    worst, row, tiny_ok, _ = fm.table_errors(got)
    t = fm.truth_table()
    print("device worst relative error %.3e at row %d (k %d, n %g, p %g); bound %.3e"
          % (worst, row, t["k"][row], t["n"][row], t["p"][row], DEVICE_BOUND))
    assert worst <= DEVICE_BOUND
    assert tiny_ok
    closed = (t["k"] <= 0) | (t["k"] > t["n"]) | (t["p"] == 0) | (t["p"] == 1)
    assert numpy.array_equal(got[closed], t["truth"][closed])
    assert same_bits(got, table_on_device())                      # the same bits on two runs


def test_one_wave_of_mixed_lanes_equals_each_lane_alone():
    """64 lanes: closed cases, one-term tails and the longest sums the limit admits (N p = 2^20,
    k at the mode: about 8,000 terms) side by side."""
    n = 2.0 ** 40
    k = numpy.empty(64, dtype=numpy.int64)
    p = numpy.empty(64)
    for lane in range(64):
        kind = lane % 4
        if kind == 0:
            k[lane], p[lane] = (0, 1e-9) if lane % 8 else (5, 0.0)
        elif kind == 1:
            k[lane], p[lane] = 2 + lane % 3, 1e-30                # N p = 1e-18: one term
        elif kind == 2:
            k[lane], p[lane] = 1048576 + lane - 30, 2.0 ** -20    # the longest in-limit sums
        else:
            k[lane], p[lane] = 1, 1e-13 * (lane + 1)
    together = bb.binomial_sf(k, n, p)
    _, terms = fm.binomial_sf(k, n, p, return_terms=True)
    assert terms.max() > 7000 and (terms == 1).any() and (terms == 0).any()
    for lane in range(64):
        alone = bb.binomial_sf(k[lane:lane + 1], n, p[lane:lane + 1])
        assert same_bits(alone, together[lane:lane + 1]), lane
    err = rel_to(together, fm.binomial_sf(k, n, p))
    print("mixed wave: max relative difference to the model %.3e" % err)
    assert err <= DEVICE_BOUND


def test_binomial_sf_above_the_limit_is_an_error_and_writes_nothing():
    lib = _lib.load()
    k = numpy.array([5, 5, 5], dtype=numpy.int64)
    p = numpy.array([1e-9, 1e-3, 1e-9])
    out = numpy.full(3, -7.0)
    rc = lib.bb_binomial_sf(k.ctypes.data_as(_lib.p_i64), 2.0 ** 40, _lib.as_f64_ptr(p),
                            _lib.as_f64_ptr(out), 3, 0)
    assert rc == _lib.BB_ERR_INVALID and "1048576" in _lib.last_error()
    assert numpy.array_equal(out, [-7.0, -7.0, -7.0])
    with pytest.raises(ValueError, match="1048576"):
        bb.binomial_sf(k, 2.0 ** 40, p)
    # at the limit itself, and p = 1 with any n, are fine
    assert bb.binomial_sf([3], 2.0 ** 40, [2.0 ** -20])[0] == 1.0
    assert bb.binomial_sf([3], 2.0 ** 40, [1.0])[0] == 1.0


# ---- 2. the dense route ----------------------------------------------------------------------------
@pytest.mark.parametrize("d", DENSE_SIZES)
def test_dense_route_equals_the_model(d):
    """A map with a dead bin, a bias outside the range, zero cells and a prior table with a zero,
    an entry that puts the prior above 1 and a NaN (none of the last two is listed); row and
    column n_bins hold NaN, -1 and inf."""
    n, m, bias = dense_case(d)
    cm = bb.ContactMap.from_matrix(m, resolution=RES)
    for min_dist, max_dist in ranges(n):
        ks = fm.in_range(n, RES, min_dist, max_dist)
        for bias_range in ((0.5, 2.0), None):
            _, observed = fm.tallies(m, n, ks)
            n_reads = float(observed.sum())
            prior = fm.decay_prior(n, n_reads, zero_at=3, above_one_at=5, nan_at=7)
            want = fm.fithic(m, bias, RES, min_dist, max_dist, bias_range=bias_range, prior=prior)
            sums = fh.diagonal_sums(cm, n)
            assert numpy.array_equal(sums[ks[0]:ks[-1] + 1], observed[ks[0]:ks[-1] + 1])
            row, col, count, p = device_list(cm, n, min_dist, max_dist, bias, bias_range, prior, n_reads)
            assert row.dtype == numpy.int32 and col.dtype == numpy.int32
            assert row.shape[0] == want["rows"].shape[0], (d, min_dist, max_dist, bias_range)
            assert numpy.array_equal(row, want["rows"]) and numpy.array_equal(col, want["cols"])
            assert numpy.array_equal(count, want["counts"])
            if n > 8 and len(ks) > 8 and bias_range is not None:
                # cells are stored at k = 3, 5 and 7; those at 5 (prior > 1) and 7 (NaN) are left out
                stored = {k: int((numpy.diagonal(m[:n, :n], k) >= 1).sum()) for k in (3, 5, 7)}
                assert min(stored.values()) > 0
                assert (col - row == 3).any() and not numpy.isin(col - row, (5, 7)).any()
            err = rel_to(p, want["p"]) if p.size else 0.0
            print("d %d range (%d, %d] bias_range %r: %d listed, p within %.3e of the model (bound %.3e)"
                  % (d, min_dist, max_dist, bias_range, p.size, err, DEVICE_BOUND))
            assert err <= DEVICE_BOUND
            again = device_list(cm, n, min_dist, max_dist, bias, bias_range, prior, n_reads)
            assert all(numpy.array_equal(a, b) for a, b in zip(again[:3], (row, col, count)))
            assert same_bits(again[3], p)
    assert same_bits(cm.to_host(), m)                              # the matrix is as it was


def test_dense_route_reads_nothing_of_row_and_column_n_bins():
    n, m, bias = dense_case(66)
    clean = m.copy()
    clean[n, :] = 0.0
    clean[:, n] = 0.0
    _, observed = fm.tallies(m, n, fm.in_range(n, RES, *FULL))
    prior = fm.decay_prior(n, observed.sum())
    a = device_list(bb.ContactMap.from_matrix(m, resolution=RES), n, 0, FULL[1], bias, (0.5, 2.0), prior,
                    float(observed.sum()))
    b = device_list(bb.ContactMap.from_matrix(clean, resolution=RES), n, 0, FULL[1], bias, (0.5, 2.0),
                    prior, float(observed.sum()))
    assert all(same_bits(x.astype(numpy.float64), y.astype(numpy.float64)) for x, y in zip(a, b))


@pytest.mark.parametrize("d", [129, 1027])
def test_fit_transform_equals_the_model(d):
    """The whole call: tallies, binning, spline and lookup on the host, the list and p on the
    device, q from the device's own p."""
    n, m, bias = dense_case(d)
    cm = bb.ContactMap.from_matrix(m, resolution=RES, KRnorm=bias)
    f = bb.FitHiC(resolution=RES, n_bins=12)
    out = f.fit_transform(cm)                                      # biases='auto': the KRnorm
    own = fm.fithic(m, bias, RES, n_bins=12)
    prior_err = float(numpy.max(numpy.abs(f.prior_by_distance_ / own["prior"] - 1)))
    print("d %d: prior table within %.3e of the model's" % (d, prior_err))
    assert prior_err <= 1e-12
    assert numpy.array_equal(f.bins_x_, own["bins_x"]) and numpy.array_equal(f.spline_x_, own["spline_x"])
    want = fm.fithic(m, bias, RES, n_bins=12, prior=f.prior_by_distance_)
    assert (f.n_reads_, f.n_tests_, f.n_listed_) == (want["n_reads"], want["n_tests"], want["rows"].shape[0])
    assert isinstance(out, bb.FithicContactMap) and out.map.shape == (f.n_listed_, 5)
    b1, b2 = out._bins()
    assert numpy.array_equal(b1, want["rows"]) and numpy.array_equal(b2, want["cols"])
    assert numpy.array_equal(out.map[:, 0], want["rows"] * RES + RES // 2)
    assert numpy.array_equal(out.map[:, 2], want["counts"])
    err = rel_to(out.map[:, 3], want["p"])
    print("d %d: %d listed of %d tests, p within %.3e of the model (bound %.3e)"
          % (d, f.n_listed_, f.n_tests_, err, DEVICE_BOUND))
    assert err <= DEVICE_BOUND
    p = out.map[:, 3]
    order = numpy.argsort(p, kind="stable")
    q = numpy.empty_like(p)
    q[order] = bb.benjamini_hochberg(p[order], f.n_tests_)
    assert same_bits(out.map[:, 4], q)
    assert numpy.array_equal(q[order], fm.bh(p[order], f.n_tests_))
    assert same_bits(cm.to_host(), m) and cm._KRexpected is None
    # the convenience, all-ones biases and a vector
    again = cm.significance(n_bins=12)
    assert same_bits(again.map, out.map)
    ones = cm.significance(n_bins=12, biases=None, bias_range=None)
    want1 = fm.fithic(m, None, RES, n_bins=12, bias_range=None)
    assert numpy.array_equal(ones._bins()[0], want1["rows"]) and numpy.array_equal(ones._bins()[1], want1["cols"])


def test_ranges_through_the_public_call():
    n, m, bias = dense_case(129)
    cm = bb.ContactMap.from_matrix(m, resolution=RES)
    with pytest.raises(ValueError, match="range"):
        cm.significance(min_dist=n * RES, max_dist=(n + 5) * RES)          # beyond the map: empty
    with pytest.raises(ValueError, match="range"):
        cm.significance(min_dist=21, max_dist=29)                          # between two diagonals
    with pytest.raises(ValueError, match="at least 4"):
        cm.significance(min_dist=10, max_dist=20, n_bins=12)               # one diagonal: one point
    f = bb.FitHiC(resolution=RES, n_bins=12, min_dist=30, max_dist=600)
    out = f.fit_transform(cm, biases=bias)
    want = fm.fithic(m, bias, RES, 30, 600, n_bins=12, prior=f.prior_by_distance_)
    k = out._bins()[1] - out._bins()[0]
    assert k.min() == 4 and k.max() == 60
    assert numpy.array_equal(out._bins()[0], want["rows"]) and numpy.array_equal(out._bins()[1], want["cols"])
    assert f.n_tests_ == sum(n - q for q in range(4, 61))


@pytest.mark.parametrize("bad", [2.5, -1.0, numpy.nan, numpy.inf])
def test_a_cell_that_is_not_a_raw_count_raises(bad):
    n, m, bias = dense_case(66)
    m = m.copy()
    m[5, 9] = m[9, 5] = bad
    cm = bb.ContactMap.from_matrix(m, resolution=RES)
    with pytest.raises(ValueError, match="raw counts"):
        cm.significance(n_bins=12, biases=bias)
    with pytest.raises(ValueError, match="raw counts"):
        device_list(cm, n, 0, FULL[1], bias, None, fm.decay_prior(n, 1000.0), 1000.0)
    # outside the range the same cell is not counted
    out = bb.FitHiC(resolution=RES, n_bins=12, min_dist=40).fit_transform(cm, biases=bias)
    assert out.map.shape[0] > 0
    if numpy.isfinite(bad):
        # (a triple's NaN is read as 0 and its infinity as the largest double: nan_to_num)
        t = fm.triples_of(m, RES, 3, duplicates=False)
        with pytest.raises(ValueError, match="raw counts"):
            bb.DeviceTriples(t, RES, 0).significance(n, n_bins=12, biases=bias)


# ---- 3. the triples route --------------------------------------------------------------------------
@pytest.mark.parametrize("d", DENSE_SIZES)
def test_triples_route_equals_the_dense_route_bit_for_bit(d):
    """The same maps as shuffled triples with duplicate pairs (the last wins) and a pair that
    touches bin n_bins."""
    n, m, bias = dense_case(d)
    t = fm.triples_of(m, RES, d)
    cm = bb.ContactMap.from_matrix(m, resolution=RES)
    scattered = bb.ContactMap.from_triples(t, RES, n)
    assert same_bits(scattered.to_host()[:n, :n], m[:n, :n])
    dev = bb.DeviceTriples(t, RES, 0)
    for min_dist, max_dist in ranges(n):
        ks = fm.in_range(n, RES, min_dist, max_dist)
        _, observed = fm.tallies(m, n, ks)
        n_reads = float(observed.sum())
        prior = fm.decay_prior(n, n_reads, zero_at=3, above_one_at=5, nan_at=7)
        assert numpy.array_equal(fh.diagonal_sums(dev, n)[ks[0]:ks[-1] + 1], observed[ks[0]:ks[-1] + 1])
        dense = device_list(cm, n, min_dist, max_dist, bias, (0.5, 2.0), prior, n_reads)
        for X in (dev, scattered):
            got = device_list(X, n, min_dist, max_dist, bias, (0.5, 2.0), prior, n_reads)
            for a, b in zip(got, dense):
                assert a.dtype == b.dtype and a.shape == b.shape
                assert numpy.array_equal(a.view(numpy.uint8), b.view(numpy.uint8)), (d, min_dist, max_dist)
    if n >= 100:
        a = dev.significance(n, n_bins=12, biases=bias)
        b = cm.significance(n_bins=12, biases=bias)
        assert same_bits(a.map, b.map)


def test_rows_on_and_past_the_segment_cut_of_the_triples_index():
    """Rows of exactly 1,023, 1,024 and 1,025 index entries and one of 2,100: the triples route,
    whose items are 1,024-entry segments of a row, against the dense route bit for bit and against
    the model cell for cell, over the full range and over one that cuts the long rows' spans."""
    m = fm.long_rows_map()
    n = m.shape[0] - 1
    entries = (m[:n, :n] != 0).sum(axis=1)
    assert [int(entries[r]) for r in (5, 400, 800, 50)] == [1023, 1024, 1025, n] and n >= 2049
    assert numpy.sort(entries)[-5] < 1023                          # every other row is one segment
    bias = fm.random_bias(n, 1)
    t = fm.triples_of(m, RES, 11)
    cm = bb.ContactMap.from_matrix(m, resolution=RES)
    dev = bb.DeviceTriples(t, RES, 0)
    for min_dist, max_dist in (FULL, (20, 15000)):
        ks = fm.in_range(n, RES, min_dist, max_dist)
        _, observed = fm.tallies(m, n, ks)
        n_reads = float(observed.sum())
        prior = fm.decay_prior(n, n_reads, zero_at=3)
        want = fm.fithic(m, bias, RES, min_dist, max_dist, prior=prior)
        dense = device_list(cm, n, min_dist, max_dist, bias, (0.5, 2.0), prior, n_reads)
        got = device_list(dev, n, min_dist, max_dist, bias, (0.5, 2.0), prior, n_reads)
        for a, b in zip(got, dense):
            assert a.dtype == b.dtype and a.shape == b.shape
            assert numpy.array_equal(a.view(numpy.uint8), b.view(numpy.uint8)), (min_dist, max_dist)
        assert numpy.array_equal(got[0], want["rows"]) and numpy.array_equal(got[1], want["cols"])
        assert numpy.array_equal(got[2], want["counts"])
        for r in (5, 400, 800, 50):                                # the long rows are on the list
            assert (got[0] == r).sum() == (want["rows"] == r).sum() > 100
        err = rel_to(got[3], want["p"])
        print("long rows, range (%d, %d]: %d listed, p within %.3e of the model (bound %.3e)"
              % (min_dist, max_dist, got[3].size, err, DEVICE_BOUND))
        assert err <= DEVICE_BOUND
    assert dev.pairs(n) == int((numpy.triu(m[:n, :n]) != 0).sum())


def test_triples_result_is_the_same_for_every_order_of_the_list():
    n, m, bias = dense_case(129)
    t = fm.triples_of(m, RES, 1, duplicates=False)
    want = None
    for seed in range(3):
        order = numpy.random.default_rng(seed).permutation(t.shape[0])
        swapped = t[order].copy()
        swapped[::2, :2] = swapped[::2, 1::-1]
        got = bb.DeviceTriples(swapped, RES, 0).significance(n, n_bins=12, biases=bias).map
        want = got if want is None else want
        assert same_bits(got, want)


def test_balance_on_the_same_handle_keeps_its_bits():
    n, m, _ = dense_case(129)
    t = fm.triples_of(m, RES, 2)
    fresh = bb.DeviceTriples(t, RES, 0).balance(n, max_iter=30)
    dev = bb.DeviceTriples(t, RES, 0)
    before = dev.balance(n, max_iter=30)
    pairs = dev.pairs(n)
    out = dev.significance(n, n_bins=12, biases=before)
    after = dev.balance(n, max_iter=30)
    assert same_bits(before, fresh) and same_bits(after, fresh) and dev.pairs(n) == pairs
    assert out.map.shape[0] > 0
    # and the other way round: the index the significance call built serves balance
    dev2 = bb.DeviceTriples(t, RES, 0)
    dev2.significance(n, n_bins=12, biases=None)
    assert same_bits(dev2.balance(n, max_iter=30), fresh)


# ---- 4. end to end, lifetimes ----------------------------------------------------------------------
def test_planted_cells_are_called_and_the_result_feeds_the_solver():
    m, b, planted = fm.planted_map()
    cm = bb.ContactMap.from_matrix(m, resolution=fm.PLANTED_RES)
    f = bb.FitHiC(None, fm.PLANTED_RES)
    out = f.fit_transform(cm, biases=b)
    called = set(map(tuple, ((out.map[out.map[:, 4] <= 0.01, :2] - fm.PLANTED_RES // 2)
                             / fm.PLANTED_RES).astype(numpy.int64).tolist()))
    want = set(map(tuple, planted.tolist()))
    print("reads %d, tests %d, listed %d; planted called %d / %d, others %d"
          % (f.n_reads_, f.n_tests_, f.n_listed_, len(called & want), len(want), len(called - want)))
    assert want <= called
    assert len(called - want) <= 1
    model = fm.planted_model()
    assert (f.n_reads_, f.n_tests_, f.n_listed_) == (model["n_reads"], model["n_tests"], model["p"].shape[0])
    assert out.contacts().shape[0] >= 24
    s = bb.StructureSolver(n_iter=3).fit(out.to_sparse("count", n_bins=fm.PLANTED_N))
    assert numpy.isfinite(s.structure_).all()


def test_a_refused_call_leaves_no_handle_and_the_next_one_works():
    n, m, bias = dense_case(129)
    cm = bb.ContactMap.from_matrix(m, resolution=RES)
    dev = bb.DeviceTriples(fm.triples_of(m, RES, 4), RES, 0)
    lib = _lib.load()
    ones = numpy.ones(n)
    heavy = numpy.full(n, 0.5)                                     # N pi = 5e6: above the limit
    for X in (cm, dev):
        owner = X._balance_target()                                # the map's own handle
        out = _lib.c_void_p(12345)
        rc = getattr(lib, owner.prefix + "significance")(
            owner._h, n, 1, n - 1, _lib.as_f64_ptr(ones), 0.5, 2.0, _lib.as_f64_ptr(heavy), 1e7,
            ctypes.byref(out))
        assert rc == _lib.BB_ERR_INVALID and "1048576" in _lib.last_error()
        assert out.value is None                                   # no handle came back
        with pytest.raises(ValueError, match="1048576"):
            fh.significance_list(X, n, 1, n - 1, ones, (0.5, 2.0), heavy, 1e7)
        with pytest.raises(ValueError):
            fh.significance_list(X, n, 5, 2, ones, (0.5, 2.0), heavy, 1e7)     # k_lo > k_hi
        with pytest.raises(ValueError):
            fh.significance_list(X, n, 1, n, ones, (0.5, 2.0), heavy, 1e7)     # k_hi = n_bins
        with pytest.raises(ValueError):
            fh.significance_list(X, n, 1, n - 1, ones, (0.5, 2.0), heavy, 0.5)  # N not whole
        res = fh.significance_list(X, n, 1, n - 1, ones, (0.5, 2.0), fm.decay_prior(n, 1e4), 1e4)
        listed, terms = res.size()
        assert listed > 0 and terms > 0 and res.read()[3].shape == (listed,)
        res.close()
        res.close()                                                # twice is fine
    assert lib.bb_sig_destroy(None) == _lib.BB_OK
