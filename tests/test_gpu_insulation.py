"""GPU: the insulation sums of a map (docs/SPEC.md 2.13) -- `ContactMap.insulation`,
`DeviceTriples.insulation`, `insulation_triples` -- bit for bit against the numpy model of
tests/_insulation_model.py, whose order of summation is the definition's
(tests/test_insulation_cpu.py shows that another order gives other bits on the wide maps used
here), and the pixel-list route bit for bit against the dense one.  Sizes and windows sit around
the constants of bb_insulation.hip, named below.  No tolerance anywhere: every comparison is of
bit patterns and exact counts."""
import numpy
import pytest

import blueberry_amd as bb
from blueberry_amd import _lib
from tests import _insulation_model as im
from tests._util import same_bits

pytestmark = pytest.mark.gpu

# the constants of bb_insulation.hip
INS_BINS = 64        # kInsBins: bins of a workgroup of the dense kernel
INS_ROWS = 16        # kInsRows: rows of a step; a workgroup has w - 1 + INS_BINS rows
INS_COLS = 128       # kInsCols: columns of a step; a workgroup has INS_BINS + w - 1 columns
INS_WAVE_ROWS = 64   # kInsWaveRows: rows of a bin the pixel-list kernel adds per chunk
TB_SEG = 1024        # kTbSeg of the index the pixel-list kernel reads (bb_triples.h)
RES = 1000

N_BINS = [1, 2, 3, 63, 64, 65, 127, 128, 129, 257, 1000, 1025]
WINDOWS = [1, 2, 3, 5, 8, 16, 33, 64, 100]        # and n_bins, n_bins + 5
OFFSETS = [0, 1, 2, 5]                            # and 2 w - 2 (one cell), 2 w - 1 and 2 w (no cell)
KINDS = ["integer", "integer-bias", "wide", "wide-bias"]


def map_of(kind, n, seed):
    M = im.integer_map(n, seed) if kind.startswith("integer") else im.wide_map(n, seed)
    return M, (im.nan_bias(n, seed + 1) if kind.endswith("bias") else None)


def check(track, want, n, w, g):
    sums, counts = want
    assert isinstance(track, bb.InsulationTrack) and (track.window, track.ignore_diags) == (w, g)
    assert track.counts.dtype == numpy.int64 and numpy.array_equal(track.counts, counts), (n, w, g)
    bad = numpy.flatnonzero(track.sums.view(numpy.uint64) != sums.view(numpy.uint64))
    assert track.sums.shape == (n,) and bad.shape[0] == 0, (n, w, g, bad[:4], track.sums[bad[:4]], sums[bad[:4]])


# ---- 1. dense, bit for bit against the model -----------------------------------------------------
@pytest.mark.parametrize("n", N_BINS)
@pytest.mark.parametrize("kind", KINDS)
def test_dense_equals_the_model(n, kind):
    M, bias = map_of(kind, n, 100 + n)
    cmap = bb.ContactMap.from_matrix(M, resolution=RES)
    seen = {}            # (a window beyond n is n's: the model's loops are the same ones)
    for w in WINDOWS + [n, n + 5]:
        for g in OFFSETS + [2 * w - 2, 2 * w - 1, 2 * w]:
            key = (min(w, n), min(g, n))
            if key not in seen:
                seen[key] = im.sums_counts(M, n, w, g, bias)
            track = cmap.insulation(w, g, bias)
            check(track, seen[key], n, w, g)
            if g == 2 * w - 2:            # the far corner (i - w + 1, i + w - 1) alone
                assert track.full_cells == 1 and (track.counts <= 1).all()
            if g >= 2 * w - 1:
                assert track.full_cells == 0 and not track.counts.any()
                assert not track.sums.view(numpy.uint64).any() and numpy.isnan(track.score).all()


def test_dense_on_a_map_of_many_workgroups():
    n, w, g = 4200, 130, 2
    M, bias = map_of("wide-bias", n, 5)
    check(bb.ContactMap.from_matrix(M).insulation(w, g, bias), im.sums_counts(M, n, w, g, bias), n, w, g)


# ---- 2. around the kernels' constants, both routes -----------------------------------------------
# rows of a workgroup: w - 1 + INS_BINS, in steps of INS_ROWS; columns: INS_BINS + w - 1, in chunks of
# INS_COLS (one chunk up to w = 65, two up to 193); rows of a bin in the pixel-list kernel: w, in
# chunks of INS_WAVE_ROWS
EDGE_WINDOWS = sorted({INS_ROWS - 1, INS_ROWS, INS_ROWS + 1, 2 * INS_ROWS, 2 * INS_ROWS + 1,
                       INS_WAVE_ROWS - 1, INS_WAVE_ROWS, INS_WAVE_ROWS + 1,
                       INS_COLS - INS_BINS, INS_COLS - INS_BINS + 1, INS_COLS - INS_BINS + 2,
                       INS_COLS - 1, INS_COLS, INS_COLS + 1, 2 * INS_WAVE_ROWS + 1,
                       2 * INS_COLS - INS_BINS, 2 * INS_COLS - INS_BINS + 1, 2 * INS_COLS - INS_BINS + 2})
EDGE_SIZES = [INS_BINS - 1, INS_BINS, INS_BINS + 1, INS_COLS - 1, INS_COLS, INS_COLS + 1,
              3 * INS_BINS, 3 * INS_BINS + 1]


@pytest.mark.parametrize("w", EDGE_WINDOWS)
def test_both_routes_around_the_kernel_constants(w):
    for n in EDGE_SIZES:
        M, bias = map_of("wide-bias", n, 1000 * w + n)
        t = im.triples_of(M, n, RES)
        cmap = bb.ContactMap.from_matrix(M, resolution=RES)
        with bb.DeviceTriples(t, RES, 0) as dev:
            for g in (0, 2):
                want = im.sums_counts(M, n, w, g, bias)
                check(cmap.insulation(w, g, bias), want, n, w, g)
                check(dev.insulation(n, w, g, bias), want, n, w, g)


@pytest.mark.parametrize("n", [TB_SEG - 1, TB_SEG, TB_SEG + 1])
def test_rows_as_long_as_an_index_segment(n):
    """Every cell stored: row 0 of the index has n entries, one below, at and above kTbSeg."""
    M, bias = map_of("wide-bias", n, n)
    M[:n, :n][M[:n, :n] == 0.0] = 1.0
    t = im.triples_of(M, n, RES)
    assert t.shape[0] == n * (n + 1) // 2
    cmap = bb.ContactMap.from_matrix(M, resolution=RES)
    with bb.DeviceTriples(t, RES, 0) as dev:
        for w, g in ((3, 0), (INS_WAVE_ROWS + 1, 2)):
            want = im.sums_counts(M, n, w, g, bias)
            check(cmap.insulation(w, g, bias), want, n, w, g)
            check(dev.insulation(n, w, g, bias), want, n, w, g)


# ---- 3. the pixel list equals the dense route ----------------------------------------------------
def messy_list(n, seed):
    """Duplicates (the last wins), stored zeros, diagonal cells, either orientation, positions
    anywhere inside their bins, and triples that touch bin n (never read)."""
    r = numpy.random.default_rng(seed)
    M = im.wide_map(n, seed)
    t = im.triples_of(M, n, RES, keep_zeros=0.3, seed=seed)
    t = t[r.random(t.shape[0]) < 0.5]
    dup = t[r.integers(0, max(t.shape[0], 1), t.shape[0] // 4)].copy()
    dup[:, 2] = r.uniform(1.0, 10.0, dup.shape[0]) * 10.0 ** r.integers(-6, 7, dup.shape[0])
    edge = numpy.stack([r.integers(0, n + 1, 9) * float(RES), numpy.full(9, n * float(RES)), numpy.full(9, 5.0)], 1)
    t = numpy.concatenate([t, dup, edge])
    t = t[r.permutation(t.shape[0])]
    flip = r.random(t.shape[0]) < 0.5
    t[flip, 0], t[flip, 1] = t[flip, 1].copy(), t[flip, 0].copy()
    t[:, :2] += r.integers(0, RES, (t.shape[0], 2))
    return t


def same_track(a, b):
    return (same_bits(a.sums, b.sums) and numpy.array_equal(a.counts, b.counts) and same_bits(a.score, b.score)
            and same_bits(a.log2, b.log2) and same_bits(a.strength, b.strength))


@pytest.mark.parametrize("n,w,g", [(1, 1, 0), (2, 3, 0), (3, 2, 1), (64, 5, 2), (65, 16, 0), (129, 10, 2),
                                   (257, 33, 2), (257, 64, 5), (257, 300, 1), (1000, 100, 2), (1025, 8, 2)])
def test_pixel_list_equals_dense_on_messy_lists(n, w, g):
    t = messy_list(n, 31 * n + w)
    dense_map = bb.ContactMap.from_triples(t, RES, n)
    M = dense_map.matrix
    for bias in (None, im.nan_bias(n, n + w)):
        dense = dense_map.insulation(w, g, bias)
        check(dense, im.sums_counts(M, n, w, g, bias), n, w, g)
        with bb.DeviceTriples(t, RES, 0) as dev:                   # a fresh handle: the index is built
            assert same_track(dev.insulation(n, w, g, bias), dense)
            assert same_track(dev.insulation(n, w, g, bias), dense)
        assert same_track(bb.insulation_triples(t, RES, n, w, g, bias), dense)


def test_pixel_list_memory_orders_and_permutations_give_the_same_bits():
    n, w, g = 257, 20, 2
    t = im.triples_of(im.wide_map(n, 77), n, RES, keep_zeros=0.2, seed=1)     # duplicate-free
    want = bb.ContactMap.from_triples(t, RES, n).insulation(w, g)
    r = numpy.random.default_rng(5)
    for trial in range(3):
        p = t[r.permutation(t.shape[0])]
        flip = r.random(p.shape[0]) < 0.5
        p[flip, 0], p[flip, 1] = p[flip, 1].copy(), p[flip, 0].copy()
        for arr in (p, numpy.asfortranarray(p), numpy.repeat(p, 2, axis=0)[::2]):
            assert same_track(bb.insulation_triples(arr, RES, n, w, g), want)


def test_pixel_list_on_a_handle_other_calls_have_used():
    n, w, g = 300, 12, 2
    M, bias, _ = im.planted_map(n, w, 9)
    t = im.triples_of(M, n, RES)
    want = bb.ContactMap.from_triples(t, RES, n)
    with bb.DeviceTriples(t, RES, 0) as dev:
        b = dev.balance(n, ignore_diags=2)
        assert same_track(dev.insulation(n, w, g, b), want.insulation(w, g, b))
        with dev.coarsen(n, 2) as pooled:                          # pooled over the same index
            assert same_track(dev.insulation(n, w, g), want.insulation(w, g, None))
            half = want.coarsen(2)
            assert same_track(pooled.insulation(150, w, g), half.insulation(w, g))
        dev.expected(n, b)
        # another n_bins: the index is rebuilt
        assert same_track(dev.insulation(n + 10, w, g), bb.ContactMap.from_triples(t, RES, n + 10).insulation(w, g))
        assert same_track(dev.insulation(n, w, g, b), want.insulation(w, g, b))


def test_an_empty_list_and_an_empty_map():
    track = bb.insulation_triples(numpy.zeros((0, 3)), RES, 50, 5)
    assert not track.sums.view(numpy.uint64).any() and track.counts[10] == 22 and (track.score[4:46] == 0).all()
    none = bb.insulation_triples(numpy.zeros((0, 3)), RES, 0, 5)
    assert none.sums.shape == (0,) and none.boundaries()[0].shape == (0,)
    assert bb.ContactMap.from_matrix(numpy.zeros((1, 1))).insulation(3).sums.shape == (0,)


# ---- 4. what is read, and what is left -----------------------------------------------------------
def test_only_the_upper_triangle_of_the_leading_block_is_read():
    n, w, g = 257, 20, 1
    M, bias = map_of("wide-bias", n, 3)
    A = M.copy()
    A[numpy.tril_indices(n + 1, -1)] = numpy.random.default_rng(0).random((n + 1) * n // 2) * 1e6
    A[n // 3, n // 4] = numpy.nan
    A[n, :] = numpy.nan
    A[:, n] = numpy.inf
    check(bb.ContactMap.from_matrix(A).insulation(w, g, bias), im.sums_counts(M, n, w, g, bias), n, w, g)


def test_the_map_stays_as_it_is_and_resident_and_a_second_call_gives_the_same_bits():
    n, w = 257, 10
    M = im.wide_map(n, 21)
    src = bb.ContactMap.from_triples(im.triples_of(M, n, RES), RES, n)
    view = src.matrix
    before = numpy.array(view)
    first = src.insulation(w)
    assert src.is_resident and src.matrix is view and same_bits(src.to_host(), before)
    for _ in range(3):
        assert same_track(src.insulation(w), first)
    assert src.n_bins == n and src._KRnorm is None


# ---- 5. poison -----------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", [(0, 0), (3, 12), (3, 13), (60, 61), (60, 62), (64, 64), (63, 70), (100, 128),
                                  (128, 128), (7, 100)])
def test_a_nan_or_an_infinity_poisons_exactly_the_bins_whose_diamond_holds_it(cell):
    n, w, g = 129, 10, 2
    M = im.wide_map(n, 3)
    clean, _ = im.sums_counts(M, n, w, g)
    r, c = cell
    hit = numpy.zeros(n, dtype=bool)
    hit[im.poisoned_bins(n, w, g, r, c)] = True
    assert hit.sum() == (0 if (c - r < g or c - r > 2 * w - 2) else min(c, r + w - 1) - max(r, c - w + 1) + 1)
    for poison in (numpy.nan, numpy.inf):
        A = M.copy()
        A[r, c] = A[c, r] = poison
        got = bb.ContactMap.from_matrix(A).insulation(w, g).sums
        assert same_bits(got[~hit], clean[~hit])
        assert (numpy.isnan(got[hit]) if poison != poison else got[hit] == numpy.inf).all()
        assert same_bits(got, im.sums_counts(A, n, w, g)[0])


def test_a_nan_cell_of_a_bin_with_a_nan_bias_poisons_nothing():
    n, w, g = 129, 10, 2
    M = im.wide_map(n, 4)
    bias = im.nan_bias(n, 8)
    dead = int(numpy.flatnonzero(numpy.isnan(bias))[0])
    want = im.sums_counts(M, n, w, g, bias)
    A = M.copy()
    A[dead, :] = A[:, dead] = numpy.nan
    check(bb.ContactMap.from_matrix(A).insulation(w, g, bias), want, n, w, g)
    assert numpy.isfinite(want[0]).all()
    # (a pixel list cannot hold one: a triple's NaN reads as 0, SPEC 2.5.3)


# ---- 6. bias='auto', and the planted map end to end ----------------------------------------------
def test_bias_auto_takes_what_balance_left():
    n, w = 300, 12
    M, _, _ = im.planted_map(n, w, 4)
    cmap = bb.ContactMap.from_matrix(M, resolution=RES)
    assert same_track(cmap.insulation(w), cmap.insulation(w, bias=None))        # no KRnorm: all ones
    b = cmap.balance(ignore_diags=2)
    auto = cmap.insulation(w)
    assert same_track(auto, cmap.insulation(w, bias=b)) and not same_bits(auto.sums, cmap.insulation(w, bias=None).sums)
    check(auto, im.sums_counts(M, n, w, 2, b), n, w, 2)
    given = bb.ContactMap.from_matrix(M, resolution=RES, KRnorm=numpy.concatenate([b, [1.0, 1.0]]))
    assert same_track(given.insulation(w), auto)
    with pytest.raises(ValueError):
        cmap.insulation(w, bias="none")


@pytest.mark.parametrize("n,w,seed", im.PLANTED)
def test_planted_map_end_to_end(n, w, seed):
    M, _, borders = im.planted_map(n, w, seed)
    cmap = bb.ContactMap.from_matrix(M, resolution=RES)
    b = cmap.balance(ignore_diags=2)
    dense = cmap.insulation(w)
    assert dense.resolution == RES and dense.n_bins == n and dense.full_cells == w * w - 3
    ok, weakest, other = im.planted_condition(*dense.boundaries(), borders)
    print("n %d w %d: weakest planted strength %.3f, strongest other %.3f" % (n, w, weakest, other))
    assert ok, (weakest, other)
    from_list = bb.insulation_triples(im.triples_of(M, n, RES), RES, n, w, bias=b)
    assert same_track(from_list, dense)
    # the map divided in place, read without a bias: the same boundaries
    cmap.balance(ignore_diags=2, apply=True)
    applied = cmap.insulation(w, bias=None)
    assert im.planted_condition(*applied.boundaries(), borders)[0]
    assert numpy.array_equal(applied.boundaries(0.5)[0], dense.boundaries(0.5)[0])


# ---- 7. refusals and the clock -------------------------------------------------------------------
def test_refusals():
    n = 64
    M = im.integer_map(n, 2)
    cmap = bb.ContactMap.from_matrix(M)
    t = im.triples_of(M, n, RES)
    for call in (lambda: cmap.insulation(0), lambda: cmap.insulation(5, -1), lambda: cmap.insulation(5, bias=numpy.ones(n - 1)),
                 lambda: cmap.insulation(5.0), lambda: cmap.insulation(5, min_valid=2.0),
                 lambda: bb.insulation_triples(t, RES, n, 0), lambda: bb.insulation_triples(t, RES, n, 5, -1),
                 lambda: bb.insulation_triples(t, RES, n, 5, bias=numpy.ones(n + 1)),
                 lambda: bb.insulation_triples(t, RES, -1, 5),
                 lambda: bb.insulation_triples(t, RES, n - 2, 5)):             # a bin outside [0, n_bins]
        with pytest.raises(ValueError):
            call()
    M[5, :] = M[:, 5] = 0.0
    for keep_stale in (False, True):
        filtered = bb.ContactMap.from_matrix(M)
        filtered.filter(0, keep_stale=keep_stale)
        with pytest.raises(ValueError):
            filtered.insulation(5)
    emptied = bb.ContactMap.from_matrix(M)
    emptied.filter(1e12)
    with pytest.raises(ValueError, match="empty"):
        emptied.insulation(5)


def test_library_argument_checks():
    n = 10
    src = bb.datatypes._DeviceMatrix(n + 1, 0)
    sums, counts = numpy.zeros(n), numpy.zeros(n, dtype=numpy.int64)
    ps, pc = _lib.as_f64_ptr(sums), counts.ctypes.data_as(_lib.p_i64)
    for nb, w, g, why in [(n, 0, 2, "window"), (n, 3, -1, "ignore_diags"), (n - 1, 3, 2, "filtered"),
                          (n + 1, 3, 2, "filtered"), (-1, 3, 2, "n_bins")]:
        assert src._status("insulation", nb, w, g, None, ps, pc) == _lib.BB_ERR_INVALID, (nb, w, g)
        assert why in _lib.last_error()
    assert src._status("insulation", n, 3, 2, None, None, pc) == _lib.BB_ERR_INVALID
    assert src._status("insulation", n, 3, 2, None, ps, pc) == _lib.BB_OK
    tr = bb.DeviceTriples(numpy.array([[0.0, 1000.0, 2.0], [9000.0, 9000.0, 1.0]]), RES, 0)
    assert tr._status("insulation", n, 0, 2, None, ps, pc) == _lib.BB_ERR_INVALID
    assert tr._status("insulation", n, 3, -2, None, ps, pc) == _lib.BB_ERR_INVALID
    assert tr._status("insulation", 5, 3, 2, None, ps, pc) == _lib.BB_ERR_INVALID and "outside" in _lib.last_error()
    assert tr._status("insulation", n, 3, 0, None, ps, pc) == _lib.BB_OK
    assert sums[0] == 2.0 and sums[1] == 2.0 and sums[9] == 1.0 and counts[0] == 3 and counts[5] == 9
    src.close()
    tr.close()


def test_kernel_ms_is_positive_after_a_call():
    n = 1025
    M = im.integer_map(n, 1)
    cmap = bb.ContactMap.from_matrix(M)
    assert cmap.insulation(10).kernel_ms > 0.0
    assert cmap._dev._get(_lib.c_dbl, "insulation_timing") > 0.0
    with bb.DeviceTriples(im.triples_of(M, n, RES), RES, 0) as dev:
        assert dev._get(_lib.c_dbl, "insulation_timing") == 0.0
        assert dev.insulation(n, 10).kernel_ms > 0.0
