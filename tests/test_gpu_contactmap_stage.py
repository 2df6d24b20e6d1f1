"""GPU: scatter, normalize, marginals and filter of the resident ContactMap at the sizes at which
their kernels change path, bit for bit.

  normalize   `bb_cm_normalize` sends d < 256 to `normalize_kernel` (32 x 32 tiles) and d >= 256
              to `normalize128_kernel` (128 x 128 tiles, one persistent workgroup per CU that
              prefetches its next tile pair while the mirror of the current one goes out; the
              loop runs only with more tile pairs than CUs: d >= 2,817 on 256 CUs).  Dense maps
              whose lower triangle is NOT the mirror of the upper one and whose row / column
              n_bins hold finite values, against `oracle.contactmap_normalize`; KR vectors whose
              products overflow, underflow and are infinite.
  marginals   `column_sums_kernel` (128 columns per workgroup, 64-row unrolled body, scalar
  / filter    tail), `keep_scan_kernel` (the count kept so far carried across 1,024-column
              chunks), `gather_kernel` (256 new columns per workgroup), against numpy's
              `sum(axis=0)` and boolean gather; and a handle taken through filter -> marginals
              -> filter -> normalize -> marginals, where the buffer keeps its first size.
  scatter     `scatter_mark_kernel` / `scatter_store_kernel` against `oracle.contactmap_scatter`:
              no triple, one, a workgroup's worth +- 1; the diagonal, the extra bin, the three
              memory layouts; repeats inside a wave, inside a workgroup and 10,000 triples
              apart; and a count whose bit pattern is an earlier triple's index + 1.
  solver      the same marks in `scatter_entries_kernel`, through `fit_triples`.

Every comparison is on values or bits, without a tolerance.  The inputs and the properties of
inputs and oracle that make a pass mean something are in tests/_stage_maps.py and
tests/test_contactmap_stage_inputs_cpu.py.

NOT covered: `gather_kernel`'s `r += gridDim.y` stride.  A band holds at most
8 Mi / d_new elements' worth of rows and the grid has min(rows, 32,768) of them in y: the stride
would be taken only by a band of more than 32,768 rows, which the bounce buffer never holds."""
import numpy
import pytest

import blueberry_amd as bb
from blueberry_amd.solver import HipEngine
from tests import _stage_maps as sm
from tests._util import cu_count

pytestmark = pytest.mark.gpu


def assert_same_bits(got, want, what, slab=1024):
    """Bit for bit, a slab of rows at a time; names the first cell that differs."""
    assert got.shape == want.shape, what
    for lo in range(0, got.shape[0], slab):
        g = numpy.ascontiguousarray(got[lo:lo + slab]).view(numpy.uint64)
        w = numpy.ascontiguousarray(want[lo:lo + slab]).view(numpy.uint64)
        if not numpy.array_equal(g, w):
            r, c = numpy.argwhere(g != w)[0]
            raise AssertionError("%s: %d cells differ in rows %d..; first [%d][%d]: got %r, want %r"
                                 % (what, int((g != w).sum()), lo, lo + r, c,
                                    got[lo + r, c], want[lo + r, c]))


# ---- normalize -----------------------------------------------------------------------------------
def normalized_on_device(m, kr, ke):
    cm = bb.ContactMap.from_matrix(m, KRnorm=kr, KRexpected=ke)
    cm.normalize()
    assert cm.is_resident
    return cm.to_host()


def check_normalize(oracle, d):
    n = d - 1
    m = sm.pin_extreme_cells(sm.dense_map(d))
    keep = m.copy()
    for family in ("plain", "extreme"):
        kr, ke = sm.KR_FAMILIES[family](n)
        want = oracle.contactmap_normalize(m, kr, ke)
        got = normalized_on_device(m, kr, ke)
        assert_same_bits(got, want, "normalize d=%d %s" % (d, family))
        if family == "extreme":
            # on the oracle's output alone: the wanted outcomes are there
            w = want[:n, :n]
            assert (numpy.abs(w) == sm.DBL_MAX).any()
            assert abs(want[6, 7]) == sm.DBL_MAX and want[38, 39] == 0.0       # x / 0, 0 / 0 (NaN)
            assert want[3, 4] == 0.0 and m[3, 4] != 0.0                         # x / inf
        # row and column n_bins come back as their own nan_to_num
        assert sm.same_bits(got[n, :], numpy.nan_to_num(m[n, :]))
        assert sm.same_bits(got[:, n], numpy.nan_to_num(m[:, n]))
    assert sm.same_bits(m, keep)


@pytest.mark.parametrize("d", sm.NORMALIZE_SIZES)
def test_normalize_dense_asymmetric_vs_oracle(oracle, d):
    """Both kernels on both sides of their switch, at multiples of the tile edges and one past
    them, and on both sides of the size at which the persistent loop starts."""
    cus = cu_count()
    if d >= 2817:
        assert sm.tile_pairs(d) > cus, "d=%d: %d tile pairs, %d CUs" % (d, sm.tile_pairs(d), cus)
        assert sm.trips(d, cus)[0] >= 2
    check_normalize(oracle, d)


def test_normalize_three_trips_and_a_ragged_last_round(oracle):
    """d = 4,225 (595 tile pairs) on 256 CUs: workgroups 0 .. 82 make three trips, the others
    two.  On a device with another CU count the size is computed from it."""
    cus = cu_count()
    d = sm.three_trip_size(cus)
    most, fewest = sm.trips(d, cus)
    print("CUs %d: d = %d, %d tile pairs, %d / %d trips" % (cus, d, sm.tile_pairs(d), most, fewest))
    assert sm.tile_pairs(d) > cus and most >= 3 and fewest == most - 1
    assert sm.tile_pairs(d) % cus != 0                      # the last round is ragged
    check_normalize(oracle, d)


@pytest.mark.parametrize("d", [257, 2817])
@pytest.mark.parametrize("family", ["plain", "extreme"])
def test_normalize_twice_and_on_two_handles(oracle, d, family):
    """The same handle normalised twice holds the oracle applied twice (the second pass reads
    what the first mirrored); two fresh handles hold the same bits as each other and the oracle."""
    n = d - 1
    m = sm.pin_extreme_cells(sm.dense_map(d))
    kr, ke = sm.KR_FAMILIES[family](n)
    once = oracle.contactmap_normalize(m, kr, ke)
    twice = oracle.contactmap_normalize(once, kr, ke)
    cm = bb.ContactMap.from_matrix(m, KRnorm=kr, KRexpected=ke)
    cm.normalize()
    first = cm.to_host()
    cm.normalize()
    assert_same_bits(first, once, "first pass")
    assert_same_bits(cm.to_host(), twice, "second pass")
    other = normalized_on_device(m, kr, ke)
    assert_same_bits(other, first, "two handles")


# ---- marginals and filter ------------------------------------------------------------------------
@pytest.mark.parametrize("d", sm.FILTER_SIZES)
def test_marginals_and_filter_at_the_kernel_edges(d):
    """63 / 64 / 65 rows: the unrolled body of column_sums_kernel does not run, runs once with no
    tail, runs once with a one-row tail; 128 / 129 and 255 / 256 / 257 columns: its workgroups
    and gather_kernel's; 1,023 / 1,024 / 1,025 and 2,048: keep_scan_kernel's chunks."""
    m = sm.ragged_map(d)
    marg = sm.filter_numpy(m, 0.0)[0]
    for name, thr in sm.thresholds(marg):
        cm = bb.ContactMap.from_matrix(m)
        assert numpy.array_equal(cm.marginals(), marg, equal_nan=True), name
        cm.filter(thr)
        _, keep, want = sm.filter_numpy(m, thr)
        assert cm.shape == want.shape and cm.n_bins == want.shape[0], name
        got = cm.to_host()
        # (a kept NaN / inf cell: rows 3, 5 against columns 2, 7 and the like)
        assert numpy.array_equal(got, want, equal_nan=True), name
        if want.shape[0]:
            with numpy.errstate(all="ignore"):
                assert numpy.array_equal(cm.marginals(), want.sum(axis=0), equal_nan=True), name


@pytest.mark.parametrize("name", sorted(sm.keep_patterns()))
def test_filter_keep_patterns_on_chunk_and_workgroup_edges(name):
    keep = sm.keep_patterns()[name]
    m = sm.masked_map(keep)
    cm = bb.ContactMap.from_matrix(m)
    assert numpy.array_equal(cm.marginals(), m.sum(axis=0))
    cm.filter(0.0)
    _, got_keep, want = sm.filter_numpy(m, 0.0)
    assert numpy.array_equal(got_keep, keep)
    assert cm.shape == want.shape
    assert numpy.array_equal(cm.to_host(), want)
    assert numpy.array_equal(cm.marginals(), want.sum(axis=0))


@pytest.mark.parametrize("d,first,second", [(1025, 600, 300), (2817, 1400, 200)])
def test_one_handle_through_filter_marginals_filter_normalize_marginals(oracle, d, first, second):
    """The buffer keeps the size it was made with; only the pitch changes.  From 1,025 the map
    stays above 256 bins (normalize128_kernel on a filtered handle); from 2,817 it ends below 256
    (normalize_kernel on a buffer of 2,817^2).  Every stage against numpy / the oracle on the
    host copy taken the same way."""
    m = sm.pipeline_map(d)
    cm = bb.ContactMap.from_matrix(m)
    thr1 = sm.quantile_threshold(m.sum(axis=0), first)
    cm.filter(thr1)
    host = sm.filter_numpy(m, thr1)[2]
    assert host.shape == (first, first) and cm.shape == host.shape and cm.is_resident
    assert numpy.array_equal(cm.to_host(), host)
    marg = host.sum(axis=0)
    assert numpy.array_equal(cm.marginals(), marg)
    thr2 = sm.quantile_threshold(marg, second)
    assert thr2 > thr1
    cm.filter(thr2)
    host = sm.filter_numpy(host, thr2)[2]
    assert host.shape == (second, second) and cm.shape == host.shape and cm.is_resident
    assert numpy.array_equal(cm.to_host(), host)
    # fresh KR vectors for the map as it is now: its last bin is the reference's extra row
    n = second - 1
    kr, ke = sm.plain_kr(n)
    cm.n_bins, cm._KRnorm, cm._KRexpected = n, kr, ke
    cm.normalize()
    host = oracle.contactmap_normalize(host, kr, ke)
    assert cm.is_resident and cm.shape == host.shape
    assert_same_bits(cm.to_host(), host, "normalize after two filters")
    assert numpy.array_equal(cm.marginals(), host.sum(axis=0))


# ---- scatter -------------------------------------------------------------------------------------
def check_scatter(oracle, rows, res, n_bins, what):
    want = oracle.contactmap_scatter(rows, res, n_bins)
    clean = numpy.nan_to_num(rows)
    regions = numpy.union1d(clean[:, 0], clean[:, 1])
    for layout, arr in sm.layouts(rows):
        cm = bb.ContactMap.from_triples(arr, res, n_bins)
        assert_same_bits(cm.to_host(), want, "%s, layout %s" % (what, layout))
        assert cm.regions.dtype == numpy.float64
        assert numpy.array_equal(cm.regions, regions), (what, layout)
    return want


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_scatter_triple_counts_around_one_workgroup(oracle, n):
    """No triple, one, and a workgroup of 256 +- 1; a tenth of the triples on the diagonal, some
    in bin n_bins (the extra row), repeated cells among them."""
    n_bins, res = 40, 5000
    rows = sm.random_triples(n, n_bins, res, seed=n)
    want = check_scatter(oracle, rows, res, n_bins, "n=%d" % n)
    assert numpy.count_nonzero(want) <= 2 * n
    if n >= 255:
        bj, bk = (rows[:, 0] // res).astype(int), (rows[:, 1] // res).astype(int)
        assert (bj == bk).any() and (bj == n_bins).any() and (bk == n_bins).any()
        assert want[n_bins, :].any() and want[:, n_bins].any() and numpy.diag(want).any()


def test_scatter_off_grid_positions_and_the_extra_bin(oracle):
    """Positions anywhere inside their bins (regions come from numpy's union1d then)."""
    n_bins, res, n = 40, 5000, 257
    rows = sm.random_triples(n, n_bins, res, seed=9)
    rows[:, 0] += numpy.arange(n) % res
    rows[::3, 1] += 1.0
    check_scatter(oracle, rows, res, n_bins, "off grid")


def test_scatter_repeats_in_one_wave_one_workgroup_and_far_apart(oracle):
    rows, pins = sm.duplicate_triples()
    want = check_scatter(oracle, rows, 5000, 300, "duplicates")
    for t1, t2, j, k in pins:
        assert want[j, k] == rows[t2, 2] == want[k, j]


@pytest.mark.parametrize("apart", [4, 768])
def test_scatter_count_with_the_bits_of_an_earlier_triples_index(oracle, apart):
    """A later triple's count has the bit pattern t1 + 1 of an earlier triple t1 of the same cell
    (a denormal): flipped orientation off the diagonal, repeated on it, inside the first 64
    triples (apart = 4) and in another workgroup (apart = 768).  The reference leaves the later
    count in both cells.  With bare integers as marks the earlier triple took such a cell for
    its own and stored over it.  Also a later count that is a NaN of that payload (-> 0)."""
    n_bins, res = 60, 1000
    rows, pins = sm.mark_collision_triples(lambda t: t + apart, 1100, n_bins, res)
    want = check_scatter(oracle, rows, res, n_bins, "mark collision, %d apart" % apart)
    for (t1, t2, j, k), later in zip(pins, (rows[pins[0][1], 2], rows[pins[1][1], 2], 0.0)):
        cells = numpy.array([want[j, k], want[k, j], later]).view(numpy.uint64)
        assert cells[0] == cells[1] == cells[2]


# ---- the solver's scatter of entries ---------------------------------------------------------------
class _Recorder(HipEngine):
    """HipEngine that, once the triples are in, reads the stored wish distances back through
    exact integer products: (D o D) @ x for integer x."""
    probe, seen = None, None

    def set_wish_triples(self, *args, **kwargs):
        HipEngine.set_wish_triples(self, *args, **kwargs)
        type(self).seen = (self.matvec_sq(type(self).probe), self.degrees())


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_fit_triples_repeated_pairs_keep_the_last_entry_exactly(oracle, dtype):
    """`scatter_entries_kernel` marks the solver's cells as the ContactMap scatter does.  Through
    `fit_triples` with kind='wish' and integer distances 0 .. 15, repeats in one wave, one
    workgroup and 10,000 entries apart, in both orientations: the stored matrix is read back as
    (D o D) @ x with integer x -- every term and partial sum an integer below 2^24, exact in
    either type and any order -- and as the per-bin count of constraints, and equals the
    oracle's scatter (a later 0 removes a pair, a later value after a 0 restores it)."""
    rows, pins = sm.duplicate_triples()
    n_bins, res = 300, 5000
    rng = numpy.random.default_rng(5)
    rows[:, 2] = rng.integers(0, 16, rows.shape[0])
    for t1, t2, j, k in pins:
        rows[t1, 2], rows[t2, 2] = 3 + (t1 % 5), (0 if t1 % 2 else 9)
    want = oracle.contactmap_scatter(rows, res, n_bins)
    numpy.fill_diagonal(want, 0.0)                               # the diagonal carries no pair
    n = n_bins + 1
    x = rng.integers(-8, 9, (n, 3)).astype(numpy.float64)
    assert 15 * 15 * 8 * n < 2 ** 24
    _Recorder.probe, _Recorder.seen = x, None
    bb.StructureSolver(n_iter=1, dtype=dtype, kind="wish", engine=_Recorder).fit_triples(
        rows, res, n_bins, init=numpy.random.default_rng(6).standard_normal((n, 3)))
    product, degrees = _Recorder.seen
    assert numpy.array_equal(product, (want * want) @ x)
    assert numpy.array_equal(degrees, (want > 0).sum(axis=1))
