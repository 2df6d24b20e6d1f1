"""CPU: the numpy model of the insulation sums (tests/_insulation_model.py, docs/SPEC.md 2.13) and
the host tail of `InsulationTrack` -- no library, no GPU.  The cumsum model equals the plain-loop
model bit for bit; the order of summation matters on the maps the GPU test uses; the closed form
of an unclipped diamond's cells equals an enumeration; a NaN poisons exactly the bins whose
diamond holds it; the minima and strengths of a track equal scipy's, bit for bit; and planted
domain borders are found."""
import numpy
import pytest

from blueberry_amd.datatypes import InsulationTrack, check_insulation_args, insulation_full_cells
from tests import _insulation_model as im
from tests._util import same_bits

CASES = [(1, 1, 0), (2, 3, 0), (65, 8, 2), (129, 33, 1), (200, 16, 2), (130, 200, 5), (64, 4, 9)]


@pytest.mark.parametrize("n,w,g", CASES)
@pytest.mark.parametrize("with_bias", [False, True])
def test_cumsum_model_equals_the_loops(n, w, g, with_bias):
    M = im.wide_map(n, 11 * n + w)
    bias = im.nan_bias(n, n + g) if with_bias else None
    sums, counts = im.sums_counts(M, n, w, g, bias)
    want_sums, want_counts = im.sums_counts_loops(M, n, w, g, bias)
    assert same_bits(sums, want_sums)
    assert counts.dtype == numpy.int64 and numpy.array_equal(counts, want_counts)
    if with_bias and n > 2:
        assert numpy.isnan(bias).any()


def test_the_order_of_summation_matters_on_the_wide_maps():
    """`block.sum()` -- numpy's pairwise order -- gives other bits than the definition's order."""
    n, w, g = 200, 16, 2
    M = im.wide_map(n, 7)
    sums, _ = im.sums_counts(M, n, w, g)
    W = im.weighted_cells(M, n, g, im.weights(n))
    other = numpy.array([W[max(0, i - w + 1):i + 1, i:min(n, i + w)].sum() for i in range(n)])
    differ = int((sums.view(numpy.uint64) != other.view(numpy.uint64)).sum())
    print("bins whose bits depend on the order: %d of %d" % (differ, n))
    assert differ > n // 4
    assert numpy.allclose(sums, other, rtol=1e-12, atol=0.0)
    # and on an integer map it does not
    Mi = im.integer_map(n, 7)
    Wi = im.weighted_cells(Mi, n, g, im.weights(n))
    other = numpy.array([Wi[max(0, i - w + 1):i + 1, i:min(n, i + w)].sum() for i in range(n)])
    assert same_bits(im.sums_counts(Mi, n, w, g)[0], other)


def test_full_cells_closed_form_equals_an_enumeration():
    assert insulation_full_cells(10, 2) == 97
    for w in range(1, 14):
        for g in range(0, 2 * w + 3):
            assert insulation_full_cells(w, g) == im.full_cells_enumerated(w, g), (w, g)
        assert insulation_full_cells(w, 2 * w - 2) == 1 and insulation_full_cells(w, 2 * w - 1) == 0


def test_counts_of_an_unclipped_diamond_are_full_cells():
    n, w, g = 129, 10, 2
    _, counts = im.sums_counts(im.integer_map(n, 1), n, w, g)
    assert (counts[w - 1:n - w + 1] == insulation_full_cells(w, g)).all()
    assert (counts[:w - 1] < insulation_full_cells(w, g)).all()


@pytest.mark.parametrize("cell", [(0, 0), (0, 5), (3, 12), (3, 13), (60, 60), (60, 61), (60, 62), (50, 59),
                                  (100, 128), (120, 128), (128, 128), (7, 100)])
def test_a_nan_poisons_exactly_the_bins_whose_diamond_holds_it(cell):
    n, w, g = 129, 10, 2
    M = im.wide_map(n, 3)
    clean, _ = im.sums_counts(M, n, w, g)
    r, c = cell
    A = M.copy()
    A[r, c] = A[c, r] = numpy.nan
    got, _ = im.sums_counts(A, n, w, g)
    hit = numpy.zeros(n, dtype=bool)
    if c - r >= g and c - r <= 2 * w - 2:
        hit[max(r, c - w + 1):min(c, r + w - 1) + 1] = True
    assert numpy.array_equal(numpy.flatnonzero(hit), im.poisoned_bins(n, w, g, r, c))
    assert numpy.isnan(got[hit]).all() and same_bits(got[~hit], clean[~hit])
    if c - r < g:
        assert not hit.any()


# ---- the host tail -------------------------------------------------------------------------------
def scipy_strength(log2):
    """NaN except at the local minima of every maximal finite run: there scipy's prominence."""
    from scipy.signal import find_peaks, peak_prominences
    out = numpy.full(log2.shape[0], numpy.nan)
    finite = numpy.isfinite(log2)
    i = 0
    while i < log2.shape[0]:
        if not finite[i]:
            i += 1
            continue
        j = i
        while j < log2.shape[0] and finite[j]:
            j += 1
        run = -log2[i:j]
        peaks, _ = find_peaks(run)
        out[i + peaks] = peak_prominences(run, peaks)[0]
        i = j
    return out


def track_of_scores(score, w=1, g=0):
    """A track whose score is `score` (NaN: no valid cell): window 1, one cell per bin."""
    score = numpy.asarray(score, dtype=numpy.float64)
    counts = (~numpy.isnan(score)).astype(numpy.int64)
    return InsulationTrack(numpy.nan_to_num(score), counts, w, g, score.shape[0], 1000)


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("kind", ["random", "quantised"])
def test_minima_and_strengths_equal_scipy(seed, kind):
    r = numpy.random.default_rng(seed)
    n = int(r.integers(3, 400))
    score = numpy.exp(r.normal(0.0, 1.0, n))
    if kind == "quantised":
        score = 2.0 ** numpy.round(numpy.cumsum(r.normal(0.0, 0.7, n)))      # plateaus, ties
    gaps = r.random(n) < 0.06
    score[gaps] = numpy.nan
    if seed % 2:
        score[:int(r.integers(0, 3))] = numpy.nan
    track = track_of_scores(score)
    assert same_bits(track.score[~gaps], score[~gaps]) and numpy.isnan(track.score[numpy.isnan(score)]).all()
    want = scipy_strength(track.log2)
    assert same_bits(track.strength, want)
    assert numpy.isfinite(want).sum() > 0
    bins, strengths = track.boundaries()
    assert bins.dtype == numpy.int64 and numpy.array_equal(bins, numpy.flatnonzero(numpy.isfinite(want)))
    assert same_bits(strengths, want[bins])
    cut = float(numpy.median(strengths))
    some, st = track.boundaries(cut)
    assert numpy.array_equal(some, bins[strengths >= cut]) and same_bits(st, strengths[strengths >= cut])


def test_plateaus_ends_and_short_runs():
    nan = numpy.nan
    # a flat minimum counts once, in its middle (floor); a plateau that reaches an end never
    t = track_of_scores([4.0, 2.0, 2.0, 2.0, 2.0, 8.0, 1.0, 1.0, nan, 1.0, 4.0, nan, 4.0, 1.0, 4.0, nan, 3.0, nan])
    bins, strengths = t.boundaries()
    assert list(bins) == [2, 13]
    assert same_bits(t.strength, scipy_strength(t.log2))
    assert strengths[0] == t.log2[0] - t.log2[2] and strengths[1] == t.log2[12] - t.log2[13]
    # nothing scored at all
    empty = track_of_scores([nan, nan, nan])
    assert numpy.isnan(empty.log2).all() and empty.boundaries()[0].shape == (0,)
    assert track_of_scores([]).boundaries()[0].shape == (0,)


def test_score_log2_and_min_valid():
    sums = numpy.array([10.0, 0.0, -3.0, 12.0, 50.0, 8.0])
    counts = numpy.array([5, 4, 3, 2, 0, 4], dtype=numpy.int64)
    t = InsulationTrack(sums, counts, 2, 0, 6, 5000, min_valid=0.75)        # full = 4: at least 3
    assert t.full_cells == 4 and (t.window, t.ignore_diags, t.n_bins, t.resolution) == (2, 0, 6, 5000)
    assert same_bits(t.score, numpy.array([2.0, 0.0, -1.0, numpy.nan, numpy.nan, 2.0]))
    assert same_bits(t.log2, numpy.array([0.0, numpy.nan, numpy.nan, numpy.nan, numpy.nan, 0.0]))
    assert t.kernel_ms == 0.0 and t.sums.dtype == numpy.float64 and t.counts.dtype == numpy.int64
    with pytest.raises(ValueError):
        InsulationTrack(sums, counts[:5], 2, 0, 6, 5000)


def test_argument_checks():
    assert check_insulation_args(10) == (10, 2, 0.66)
    assert check_insulation_args(numpy.int64(3), 0, 1) == (3, 0, 1.0)
    for bad in [(0,), (-1,), (2.0,), (True,), ("3",), (3, -1), (3, 1.5), (3, False), (3, 2, -0.1), (3, 2, 1.5),
                (3, 2, numpy.nan)]:
        with pytest.raises(ValueError):
            check_insulation_args(*bad)


# ---- planted domains -----------------------------------------------------------------------------
@pytest.mark.parametrize("n,w,seed", im.PLANTED)
def test_planted_borders_are_found_on_the_model_track(n, w, seed):
    M, bias, borders = im.planted_map(n, w, seed)
    assert borders.shape[0] >= 3
    sums, counts = im.sums_counts(M, n, w, 2, bias)
    bins, strengths = InsulationTrack(sums, counts, w, 2, n, 10000).boundaries()
    ok, weakest, other = im.planted_condition(bins, strengths, borders)
    print("n %d w %d: %d borders, weakest planted strength %.3f, strongest other %.3f"
          % (n, w, borders.shape[0], weakest, other))
    assert ok, (weakest, other)
