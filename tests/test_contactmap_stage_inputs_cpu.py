"""CPU: the preconditions of tests/test_gpu_contactmap_stage.py.  Those tests compare bits; what
makes a bit-for-bit pass mean something is a property of their INPUTS (tests/_stage_maps.py) and
of the oracle: a lower triangle that is not the upper one's mirror, divisors that overflow and
underflow where they are meant to, sizes that do reach the persistent loop, a count that is
another triple's mark.  This file asserts those properties, so that a change to a generator
cannot quietly turn a sharp test into a blunt one.  Nothing here calls the library."""
import numpy
import pytest

from tests import _stage_maps as sm


# ---- normalize -----------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [128, 257, 513])
def test_poison_lower_triangle_differs_from_the_mirrored_upper_in_every_cell(d):
    m = sm.dense_map(d)
    n = d - 1
    blk = m[:n, :n]
    low = numpy.tri(n, n, -1, dtype=bool)
    assert sm.same_bits(blk[low], sm.poison(d)[:n, :n][low])
    assert numpy.isfinite(blk[low]).all() and numpy.unique(blk[low]).size == int(low.sum())
    assert (blk[low] != blk.T[low]).all()                      # NaN != x as well
    # no divisor of the tests can make an upper cell equal the poison below it either way round
    for family in sm.KR_FAMILIES.values():
        kr, ke = family(n)
        want, _ = sm.normalize_numpy(m, kr, ke)
        assert (want[:n, :n][low] != blk[low]).all()
    # the upper triangle: many orders of magnitude, both signs, every special
    up = blk[numpy.triu(numpy.ones((n, n), dtype=bool))]
    fin = up[numpy.isfinite(up) & (numpy.abs(up) > 1e-300)]
    assert numpy.log10(numpy.abs(fin).max() / numpy.abs(fin).min()) > 15
    assert (fin > 0).any() and (fin < 0).any()
    bits = up.view(numpy.uint64)
    for special in (0.0, -0.0, numpy.inf, -numpy.inf, 5e-324, -5e-324, 1e-310):
        assert (bits == numpy.array([special]).view(numpy.uint64)[0]).any(), special
    assert numpy.isnan(up).any()
    # row and column n_bins: different from each other, finite values, NaN and both infinities
    row, col = m[n, :n], m[:n, n]
    assert not numpy.array_equal(row, col, equal_nan=True)
    for line in (row, col):
        assert numpy.isfinite(line).any() and numpy.isnan(line).any()
        assert (line == numpy.inf).any() and (line == -numpy.inf).any()


@pytest.mark.parametrize("family", ["plain", "extreme"])
@pytest.mark.parametrize("d", [129, 257, 385])
def test_oracle_normalize_equals_the_numpy_statement_on_the_asymmetric_map(oracle, d, family):
    """The oracle reads the upper triangle only, overwrites the lower one, leaves row and column
    n_bins to nan_to_num alone and multiplies left to right: bit for bit the numpy statement."""
    n = d - 1
    m = sm.pin_extreme_cells(sm.dense_map(d))
    kr, ke = sm.KR_FAMILIES[family](n)
    assert not (kr == 0.0).any() and not (ke == 0.0).any()     # ContactMap.normalize refuses zeros
    want = oracle.contactmap_normalize(m, kr, ke)
    stated, _ = sm.normalize_numpy(m, kr, ke)
    assert sm.same_bits(want, stated)
    assert sm.same_bits(want[n, :], numpy.nan_to_num(m[n, :]))
    assert sm.same_bits(want[:, n], numpy.nan_to_num(m[:, n]))
    assert sm.same_bits(want[:n, :n], want[:n, :n].T.copy())
    assert numpy.isfinite(want).all()
    # another association of the divisor is another matrix (extreme), the plain one is not
    # sensitive to it everywhere either: the tests can tell
    i = numpy.arange(n)
    with numpy.errstate(all="ignore"):
        other = kr[:, None] * (kr[None, :] * ke[numpy.abs(i[None, :] - i[:, None])])
        alt = numpy.nan_to_num(numpy.triu(m[:n, :n] / other))
    assert not sm.same_bits(alt, numpy.triu(want[:n, :n]))


@pytest.mark.parametrize("d", [129, 257, 2817])
def test_extreme_vectors_give_every_special_outcome(oracle, d):
    """On the oracle's output alone: a +-DBL_MAX, a 0 that came from NaN and a 0 that came from
    x / inf inside the n_bins block; the left-to-right overflow, and the underflow to 0 against a
    non-zero and a zero numerator, at their pinned cells."""
    n = d - 1
    m = sm.pin_extreme_cells(sm.dense_map(d))
    kr, ke = sm.extreme_kr(n)
    want = oracle.contactmap_normalize(m, kr, ke)
    den = sm.divisor(kr, ke)
    up = numpy.triu(numpy.ones((n, n), dtype=bool))
    x, w = m[:n, :n], want[:n, :n]
    with numpy.errstate(all="ignore"):
        quo = x / den
    assert (up & (w == sm.DBL_MAX)).any() and (up & (w == -sm.DBL_MAX)).any()
    assert (up & numpy.isnan(quo) & (w == 0.0)).any()
    assert (up & numpy.isinf(den) & numpy.isfinite(x) & (x != 0.0) & (w == 0.0)).any()
    # left to right the divisor of [3][4] is infinite; any other association gives 1e100
    with numpy.errstate(all="ignore"):
        assert kr[3] * kr[4] * ke[1] == numpy.inf and numpy.isfinite(kr[3] * (kr[4] * ke[1]))
    assert numpy.isfinite(m[3, 4]) and m[3, 4] != 0.0 and want[3, 4] == 0.0 and want[4, 3] == 0.0
    assert want[35, 36] == 0.0 and numpy.signbit(want[35, 36])          # -7 / +inf = -0.0
    # the divisor of [6][7] underflows to 0: x / 0 and 0 / 0
    assert kr[6] * kr[7] == 0.0 and den[6, 7] == 0.0 and den[38, 39] == 0.0
    assert m[6, 7] != 0.0 and abs(want[6, 7]) == sm.DBL_MAX and want[7, 6] == want[6, 7]
    assert m[38, 39] == 0.0 and want[38, 39] == 0.0
    # negative, infinite and denormal entries all occur, and an infinite product
    assert (kr < 0).any() and numpy.isinf(kr).any() and (numpy.abs(kr) < 2.3e-308).any()
    assert (ke < 0).any() and (numpy.abs(ke) < 2.3e-308).any()
    assert numpy.isinf(den[up]).any()
    # and a fair share of ordinary cells is left
    assert (up & numpy.isfinite(quo) & (quo != 0.0) & (numpy.abs(w) < sm.DBL_MAX)).sum() > up.sum() // 10


def test_tile_pair_counts_at_the_named_sizes_for_256_cus():
    cus = 256
    assert [sm.tile_pairs(d) for d in sm.PERSISTENT_SIZES] == [253, 276, 300]
    assert sm.tile_pairs(sm.THREE_TRIP_SIZE) == 595 == 2 * cus + 83
    assert sm.tile_pairs(2816) <= cus < sm.tile_pairs(2817)            # the loop starts at 2,817
    assert sm.trips(2816, cus) == (1, 1) and sm.trips(2817, cus) == (2, 1)
    assert sm.trips(2945, cus) == (2, 1)
    assert sm.trips(sm.THREE_TRIP_SIZE, cus) == (3, 2)                 # ragged last round
    assert sm.has_three_trips(sm.THREE_TRIP_SIZE, cus) and sm.three_trip_size(cus) == sm.THREE_TRIP_SIZE
    for other in (64, 120, 228, 304, 595):
        d = sm.three_trip_size(other)
        most, fewest = sm.trips(d, other)
        assert sm.has_three_trips(d, other) and most >= 3 and fewest == most - 1 and d % 128 == 1
    # the switch and the tile edges
    assert all(d < sm.BIG_FROM for d in sm.SMALL_SIZES) and sm.SWITCH_SIZES == [255, 256, 257]
    assert [sm.tile_pairs(d) for d in sm.TILE_EDGE_SIZES] == [6, 10, 10, 15]
    assert sm.tile_pairs(255, sm.TILE) == 36 and sm.tile_pairs(129, sm.TILE) == 15


# ---- scatter -------------------------------------------------------------------------------------
@pytest.mark.parametrize("apart", [4, 768])
def test_the_denormal_count_is_the_earlier_triples_mark_and_the_oracle_keeps_the_later(oracle, apart):
    n, n_bins, res = 1100, 60, 1000
    rows, pins = sm.mark_collision_triples(lambda t: t + apart, n, n_bins, res)
    assert [p[:2] for p in pins] == [(5, 5 + apart), (20, 20 + apart), (30, 30 + apart)]
    if apart == 4:
        assert all(t2 < 64 for _, t2, _, _ in pins)                   # one wave
    else:
        assert all(t1 // 256 != t2 // 256 for t1, t2, _, _ in pins)   # two workgroups
    want = oracle.contactmap_scatter(rows, res, n_bins)
    for (t1, t2, j, k), is_nan in zip(pins, (False, False, True)):
        bits = int(rows[t2:t2 + 1, 2].view(numpy.uint64)[0])
        assert bits & 0xFFFFFFFF == t1 + 1 and (bits >> 32 == 0xFFF80000 if is_nan else bits == t1 + 1)
        assert numpy.isnan(rows[t2, 2]) == is_nan
        later = 0.0 if is_nan else rows[t2, 2]                        # nan_to_num
        assert later != 0.0 or is_nan
        assert int(rows[t1, 0] // res) == j and int(rows[t1, 1] // res) == k
        assert {int(rows[t2, 0] // res), int(rows[t2, 1] // res)} == {j, k}
        for cell in (want[j, k], want[k, j]):
            assert numpy.array([cell]).view(numpy.uint64)[0] == numpy.array([later]).view(numpy.uint64)[0]
        # no other triple names the cell
        bj, bk = (rows[:, 0] // res).astype(int), (rows[:, 1] // res).astype(int)
        named = ((bj == j) & (bk == k)) | ((bj == k) & (bk == j))
        assert sorted(numpy.flatnonzero(named)) == [t1, t2]


def test_duplicate_triples_pin_their_cells(oracle):
    rows, pins = sm.duplicate_triples()
    res, n_bins = 5000, 300
    want = oracle.contactmap_scatter(rows, res, n_bins)
    bj, bk = (rows[:, 0] // res).astype(int), (rows[:, 1] // res).astype(int)
    assert len(pins) == 9
    spans = set()
    for t1, t2, j, k in pins:
        named = ((bj == j) & (bk == k)) | ((bj == k) & (bk == j))
        assert sorted(numpy.flatnonzero(named)) == [t1, t2]
        assert want[j, k] == rows[t2, 2] == want[k, j] and rows[t1, 2] != rows[t2, 2]
        spans.add("wave" if t2 < 64 else "workgroup" if t2 < 256 else "far")
        assert t1 < 64 and (t2 < 256 or t2 - t1 == 10000)
    assert spans == {"wave", "workgroup", "far"}
    assert sum(1 for t1, t2, j, k in pins if j == k) == 3
    assert sum(1 for t1, t2, j, k in pins if j != k and bj[t1] != bj[t2]) == 3      # flipped
    # the background repeats cells too, in both orientations
    key = numpy.minimum(bj, bk) * 1000 + numpy.maximum(bj, bk)
    assert numpy.unique(key).size < 0.95 * key.size


# ---- marginals and filter ------------------------------------------------------------------------
def test_keep_patterns_hit_their_chunk_and_workgroup_edges():
    pats = sm.keep_patterns()
    d = sm.KEEP_EDGE
    assert d > 2048 and d % 1024
    first = {k: int(numpy.flatnonzero(v)[0]) for k, v in pats.items()}
    last = {k: int(numpy.flatnonzero(v)[-1]) for k, v in pats.items()}
    assert first["first_kept_is_1024"] == 1024 and first["first_kept_is_1023"] == 1023
    assert last["last_kept_is_1023"] == 1023 and last["last_kept_is_1024"] == 1024
    assert first["first_kept_is_2048"] == 2048 and last["first_kept_is_2048"] == d - 1
    c = pats["chunk0_empty_chunk1_full"]
    assert not c[:1024].any() and c[1024:2048].all() and not c[2048:].any()
    counts = {k: int(v.sum()) for k, v in pats.items()}
    assert counts["kept_512_scattered"] == 512 and counts["kept_256_across_a_chunk_edge"] == 256
    assert counts["chunk0_empty_chunk1_full"] == 1024 and counts["last_kept_is_1023"] == 1024
    assert counts["kept_257"] == 257
    k = pats["kept_256_across_a_chunk_edge"]
    assert k[:1024].any() and k[1024:].any()
    assert [int(x) for x in numpy.flatnonzero(pats["one_per_chunk"])] == [1023, 2047, d - 1]
    for name, keep in pats.items():
        m = sm.masked_map(keep)
        marg, got_keep, want = sm.filter_numpy(m, 0.0)
        assert numpy.array_equal(got_keep, keep), name
        assert want.shape == (counts[name],) * 2 and numpy.array_equal(m, m.T)
        assert want.flags.c_contiguous


def test_filter_reference_sums_its_columns_in_row_order():
    """The marginals of a filtered map are compared with `sum(axis=0)` of the host reference:
    that is the sum in row order -- what the device computes -- only for a C-contiguous array."""
    m = sm.pipeline_map(1025)
    _, keep, want = sm.filter_numpy(m, sm.quantile_threshold(m.sum(axis=0), 600))
    assert want.flags.c_contiguous and numpy.array_equal(want, m[keep][:, keep])
    acc = numpy.zeros(want.shape[0])
    for row in want:
        acc = acc + row
    assert numpy.array_equal(acc, want.sum(axis=0))
    assert not numpy.array_equal(acc, m[keep][:, keep].sum(axis=0))      # F-ordered: another order


@pytest.mark.parametrize("d", [63, 257, 1025])
def test_ragged_map_and_thresholds_cut_where_they_should(d):
    m = sm.ragged_map(d)
    marg, _, _ = sm.filter_numpy(m, 0.0)
    assert numpy.isnan(marg).sum() == 2 and numpy.isinf(marg).sum() == 2
    fin = numpy.abs(m[numpy.isfinite(m)])
    assert numpy.log10(fin.max() / fin[fin > 0].min()) > 10
    # the order of a column's additions matters: the reversed order gives other bits
    assert not numpy.array_equal(marg, m[::-1].sum(axis=0), equal_nan=True)
    kept = {name: int(sm.filter_numpy(m, thr)[1].sum()) for name, thr in sm.thresholds(marg)}
    assert kept["none"] == 0 and kept["all"] == d - 2
    assert kept["above"] == kept["at"] and kept["below"] == kept["at"] + 1
    assert 0 < kept["median"] < d - 2


@pytest.mark.parametrize("d,first,second", [(1025, 600, 300), (2817, 1400, 200)])
def test_pipeline_map_filters_to_the_sizes_the_chain_needs(d, first, second):
    m = sm.pipeline_map(d)
    marg, keep, f1 = sm.filter_numpy(m, sm.quantile_threshold(m.sum(axis=0), first))
    assert f1.shape == (first, first) and numpy.log10(marg.max() / marg.min()) > 2
    marg2, keep2, f2 = sm.filter_numpy(f1, sm.quantile_threshold(f1.sum(axis=0), second))
    assert f2.shape == (second, second)
    assert (first >= sm.BIG_FROM) and ((second >= sm.BIG_FROM) == (d == 1025))
    assert sm.quantile_threshold(f1.sum(axis=0), second) > sm.quantile_threshold(m.sum(axis=0), first)
