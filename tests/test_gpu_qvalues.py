"""GPU: the q-value rule of docs/SPEC.md 2.9.7 -- key, stable radix sort, Benjamini-Hochberg scan,
scatter -- through `q_values` (host in, host out), through the resident list of a significance call
(`bb_sig_q_values`, `bb_sig_read_q`, `bb_sig_select`) and through `FitHiC.fit_transform`.

The oracle is numpy's stable argsort and the library's own `benjamini_hochberg` on the sorted
values, which the golden vectors pin: q by bits, the order exactly.  (`fm.bh` has no seed of 0.0
and other NaN and -0.0 behaviour: it is used on values in [0, 1] alone.)

Lengths, by structure: a wave is 64 values (0, 1, 2, 63, 64, 65); a round of the sort's scatter 256
(255, 256, 257); a workgroup of the scan 1,024 (1,023, 1,024, 1,025); a tile of the sort 4,096
(4,095, 4,096, 4,097, and 8,193: a third tile of one value); 262,145 is 256 x 1,024 + 1 -- the
second chunk of the scan's pass over its workgroups' summaries -- and 65 sort tiles.  Families
(tests/_qvalue_model.py): random 64-bit patterns (every digit of all eight passes varies; NaNs,
negatives), an alphabet of specials with heavy ties, all equal, uniform, values one ulp apart
(only the lowest digit differs), sorted and reversed.  Everything is exact: no tolerance."""
import ctypes

import numpy
import pytest

import blueberry_amd as bb
from blueberry_amd import _lib
from blueberry_amd import fithic as fh
from tests import _fithic_model as fm
from tests import _qvalue_model as qm
from tests._util import same_bits

pytestmark = pytest.mark.gpu

RES = 10
FULL = (0, 10000000)
LENGTHS = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8193, 262145]


def host_route(p, n_tests):
    """(q, order) as `fit_transform` computed them before the device sort."""
    order = numpy.argsort(p, kind="stable")
    q = numpy.empty_like(p)
    if p.shape[0]:
        q[order] = bb.benjamini_hochberg(p[order], n_tests)
    return q, order


# ---- 1. q_values: host in, host out ----------------------------------------------------------------
@pytest.mark.parametrize("m", LENGTHS)
def test_q_values_equal_the_host_route_bit_for_bit(m):
    for name in qm.FAMILIES:
        p = qm.family(name, m)
        n_tests = m + 7
        want_q, want_order = host_route(p, n_tests)
        q, order = bb.q_values(p, n_tests, return_order=True)
        assert order.dtype == numpy.int64 and numpy.array_equal(order, want_order), (name, m)
        assert q.dtype == numpy.float64 and same_bits(q, want_q), (name, m)
        assert same_bits(bb.q_values(p, n_tests), q), (name, m)    # without the order; a second run
        if name in ("uniform", "sorted", "reversed", "equal") and m:
            assert numpy.array_equal(q[order], fm.bh(p[order], n_tests)), (name, m)


def test_q_values_shapes_default_n_tests_and_dtypes():
    p = qm.family("uniform", 6 * 35).reshape(6, 35)
    q = bb.q_values(p)
    assert q.shape == (6, 35) and q.dtype == numpy.float64
    want, _ = host_route(p.reshape(-1), p.size)                    # n_tests = the number of values
    assert same_bits(q.reshape(-1), want)
    assert same_bits(bb.q_values(p.T), host_route(numpy.ascontiguousarray(p.T).reshape(-1), p.size)[0]
                     .reshape(35, 6))                              # taken in C order
    assert bb.q_values([]).shape == (0,)
    assert bb.q_values(0.5).shape == () and bb.q_values(0.5) == 0.5
    ints = numpy.array([[1, 0], [0, 1]])
    assert same_bits(bb.q_values(ints, 3), bb.q_values(ints.astype(numpy.float64), 3))
    f32 = p.astype(numpy.float32)
    assert same_bits(bb.q_values(f32), bb.q_values(f32.astype(numpy.float64)))
    assert same_bits(bb.q_values(p, 0), numpy.zeros_like(p))       # no tests: p * 0


def test_q_values_refusals_at_the_c_abi():
    lib = _lib.load()
    p = numpy.array([0.5, 0.25])
    q = numpy.full(2, -7.0)
    assert lib.bb_q_values(_lib.as_f64_ptr(p), -1, 2, _lib.as_f64_ptr(q), None, 0) == _lib.BB_ERR_INVALID
    assert lib.bb_q_values(_lib.as_f64_ptr(p), 2 ** 32, 2, _lib.as_f64_ptr(q), None, 0) == _lib.BB_ERR_INVALID
    assert "2^32" in _lib.last_error()
    assert lib.bb_q_values(_lib.as_f64_ptr(p), 2, -1, _lib.as_f64_ptr(q), None, 0) == _lib.BB_ERR_INVALID
    assert lib.bb_q_values(None, 2, 2, _lib.as_f64_ptr(q), None, 0) == _lib.BB_ERR_INVALID
    assert numpy.array_equal(q, [-7.0, -7.0])
    assert lib.bb_q_values(None, 0, 0, None, None, 0) == _lib.BB_OK           # m = 0 is fine
    assert lib.bb_q_values(_lib.as_f64_ptr(p), 2, 2, _lib.as_f64_ptr(q), None, 0) == _lib.BB_OK
    assert numpy.array_equal(q, [0.5, 0.5])


# ---- 2. the resident list --------------------------------------------------------------------------
def dense_case(d):
    """(n, the (n + 1)^2 map, the bias vector) of edge d, as tests/test_gpu_significance.py draws
    them; d = 0: `fm.long_rows_map`."""
    if d == 0:
        m = fm.long_rows_map()
        return m.shape[0] - 1, m, fm.random_bias(m.shape[0] - 1, 1)
    n = d - 1
    return n, fm.random_map(n, 4 if d == 3 else d), fm.random_bias(n, d)


def resident_list(X, n, m, bias):
    """The list of map `m` over the full range on handle X, and its number of tests."""
    ks = fm.in_range(n, RES, *FULL)
    possible, observed = fm.tallies(m, n, ks)
    n_reads = float(observed.sum())
    prior = fm.decay_prior(n, n_reads, zero_at=3)
    res = fh.significance_list(X, n, ks[0], ks[-1], numpy.ascontiguousarray(bias), (0.5, 2.0), prior, n_reads)
    return res, int(sum(possible[k] for k in ks))


@pytest.mark.parametrize("d", [3, 129, 1027, 0])
def test_handle_route_equals_the_host_route_on_both_list_routes(d):
    n, m, bias = dense_case(d)
    cm = bb.ContactMap.from_matrix(m, resolution=RES)
    dev = bb.DeviceTriples(fm.triples_of(m, RES, 11 if d == 0 else d), RES, 0)
    want = None
    for X in (cm, dev):
        res, n_tests = resident_list(X, n, m, bias)
        try:
            row, col, count, p = res.read()
            sort_ms, scan_ms = res.q_values(n_tests)
            q = res.read_q()
            if want is None:
                want = host_route(p, n_tests)[0]
                assert p.shape[0] > (0 if d == 3 else 1000)
                order = numpy.argsort(p, kind="stable")
                assert numpy.array_equal(q[order], fm.bh(p[order], n_tests))   # p lies in [0, 1]
            assert same_bits(q, want), d
            assert p.shape[0] == 0 or (sort_ms > 0.0 and scan_ms > 0.0)
            res.q_values(2 * n_tests)                              # again: recomputed ...
            assert same_bits(res.read_q(), host_route(p, 2 * n_tests)[0])
            res.q_values(n_tests)
            assert same_bits(res.read_q(), want)                   # ... and the same bits
            again = res.read()                                     # the list is as it was
            assert all(numpy.array_equal(a.view(numpy.uint8), b.view(numpy.uint8))
                       for a, b in zip(again, (row, col, count, p)))
        finally:
            res.close()


@pytest.fixture(scope="module")
def listed():
    """The list of dense_case(1027) with its q-values, and what the host selects from."""
    n, m, bias = dense_case(1027)
    res, n_tests = resident_list(bb.ContactMap.from_matrix(m, resolution=RES), n, m, bias)
    res.q_values(n_tests)
    cells = res.read() + (res.read_q(),)
    yield res, cells
    res.close()


def check_selection(res, cells, q_max):
    q = cells[4]
    keep = q <= q_max
    sel = res.select(q_max)
    try:
        assert sel.size() == (int(keep.sum()), 0)
        got = sel.read() + (sel.read_q(),)
        for a, b in zip(got, cells):
            assert a.dtype == b.dtype and numpy.array_equal(a.view(numpy.uint8), b[keep].view(numpy.uint8))
    finally:
        sel.close()
        sel.close()
    return int(keep.sum())


def test_select_below_at_and_above_the_q_values(listed):
    res, cells = listed
    q = cells[4]
    assert q.shape[0] > 4096 and not numpy.isnan(q).any()
    below = float(numpy.nextafter(q.min(), -numpy.inf))                    # (q.min() is 0: a prior of 0)
    assert check_selection(res, cells, below) == 0                         # below every q: empty
    assert check_selection(res, cells, -numpy.inf) == 0
    assert check_selection(res, cells, 1.0) == q.shape[0]                  # everything
    assert check_selection(res, cells, numpy.inf) == q.shape[0]
    at = float(numpy.sort(q)[q.shape[0] // 3])                             # a value that occurs
    k = check_selection(res, cells, at)
    assert k >= q.shape[0] // 3 + 1 and k == int((q < at).sum()) + int((q == at).sum())   # inclusive
    assert 0 < check_selection(res, cells, float(numpy.median(q))) < q.shape[0]
    assert check_selection(res, cells, float(q.min())) >= 1


def test_select_of_a_selection_and_of_an_empty_one(listed):
    res, cells = listed
    q = cells[4]
    cut = float(numpy.median(q))
    sel = res.select(cut)
    try:
        kept = tuple(c[q <= cut] for c in cells)
        lower = float(numpy.sort(kept[4])[kept[4].shape[0] // 2])
        assert check_selection(sel, kept, lower) > 0
        empty = sel.select(-1.0)
        assert empty.size() == (0, 0) and empty.read_q().shape == (0,) and empty.read()[0].shape == (0,)
        assert empty.q_values(5) == (0.0, 0.0) and empty.read_q().shape == (0,)   # nothing to sort
        none = empty.select(1.0)
        assert none.size() == (0, 0)
        none.close()
        empty.close()
    finally:
        sel.close()


def test_refusals_leave_the_handle_working():
    n, m, bias = dense_case(129)
    res, n_tests = resident_list(bb.ContactMap.from_matrix(m, resolution=RES), n, m, bias)
    lib = _lib.load()
    try:
        listed_cells = res.size()[0]
        out = _lib.c_void_p(12345)
        assert lib.bb_sig_select(res._h, 0.5, ctypes.byref(out)) == _lib.BB_ERR_STATE   # before q
        assert out.value is None
        qbuf = numpy.full(listed_cells, -7.0)
        assert lib.bb_sig_read_q(res._h, _lib.as_f64_ptr(qbuf)) == _lib.BB_ERR_STATE
        assert (qbuf == -7.0).all()
        with pytest.raises(RuntimeError, match="q-values"):
            res.select(0.5)
        with pytest.raises(RuntimeError, match="q-values"):
            res.read_q()
        with pytest.raises(ValueError):
            res.q_values(-1)
        res.q_values(n_tests)
        out = _lib.c_void_p(12345)
        assert lib.bb_sig_select(res._h, float("nan"), ctypes.byref(out)) == _lib.BB_ERR_INVALID
        assert out.value is None and "NaN" in _lib.last_error()
        with pytest.raises(ValueError, match="NaN"):
            res.select(numpy.nan)
        # after the refusals the handle still works
        cells = res.read() + (res.read_q(),)
        assert same_bits(cells[4], host_route(cells[3], n_tests)[0])
        assert check_selection(res, cells, 1.0) == listed_cells
    finally:
        res.close()


# ---- 3. fit_transform ------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [129, 1027])
def test_fit_transform_with_q_max_equals_the_selected_rows(d):
    n, m, bias = dense_case(d)
    cm = bb.ContactMap.from_matrix(m, resolution=RES, KRnorm=bias)
    f = bb.FitHiC(resolution=RES, n_bins=12)
    full = f.fit_transform(cm)
    assert f.n_selected_ == f.n_listed_ == full.map.shape[0] and f.sort_ms_ > 0 and f.bh_ms_ > 0
    # without q_max: q is q_values of the p column
    assert same_bits(full.map[:, 4], bb.q_values(full.map[:, 3], f.n_tests_))
    listed_cells = f.n_listed_
    for q_max in (0.01, float(numpy.sort(full.map[:, 4])[full.map.shape[0] // 4])):
        want = full.map[full.map[:, 4] <= q_max]
        g = bb.FitHiC(resolution=RES, n_bins=12)
        got = g.fit_transform(cm, q_max=q_max)
        print("d %d q_max %g: %d selected of %d listed" % (d, q_max, g.n_selected_, g.n_listed_))
        assert isinstance(got, bb.FithicContactMap) and got.map.shape == want.shape
        assert same_bits(got.map, want)
        assert g.n_selected_ == want.shape[0] and g.n_listed_ == listed_cells
        assert same_bits(cm.significance(n_bins=12, q_max=q_max).map, want)
    dev = bb.DeviceTriples(fm.triples_of(m, RES, d), RES, 0)
    q_max = float(numpy.sort(full.map[:, 4])[full.map.shape[0] // 4])
    assert same_bits(dev.significance(n, n_bins=12, biases=bias, q_max=q_max).map,
                     full.map[full.map[:, 4] <= q_max])


def test_planted_cells_are_what_q_max_selects():
    m, b, planted = fm.planted_map()
    cm = bb.ContactMap.from_matrix(m, resolution=fm.PLANTED_RES)
    full = bb.FitHiC(None, fm.PLANTED_RES).fit_transform(cm, biases=b)
    f = bb.FitHiC(None, fm.PLANTED_RES)
    got = f.fit_transform(cm, biases=b, q_max=bb.Q_LOWER_BOUND)
    want = full.map[full.map[:, 4] <= bb.Q_LOWER_BOUND]
    assert same_bits(got.map, want)
    assert planted.shape[0] <= f.n_selected_ == want.shape[0] < f.n_listed_ == full.map.shape[0]
