"""The model of tests/_input_model.py on hand-made cases and against the CPU oracle where the
oracle has the same loop, and the exactness preconditions of every case of
tests/test_gpu_input_routes.py: a case whose sums are not exact has to fail here, not on the
device."""
import numpy
import pytest

from tests import _input_model as im
from tests import _oracle
from tests import _spectral_model as sm

DTYPES = ("float32", "float64")
_ids = lambda c: "%s-%d" % c                              # noqa: E731


# ---- the rules on hand-made cases ----------------------------------------------------------------
def test_nan_to_num_and_truncation():
    a = im.nan_to_num([numpy.nan, numpy.inf, -numpy.inf, -0.5, 3.0])
    assert numpy.array_equal(a, [0.0, im.DBL_MAX, -im.DBL_MAX, -0.5, 3.0])
    pos = [-4999.0, -0.5, numpy.nan, 0.0, 4999.0, 4999.99, 5000.0, 9999.5, 3 * 5000 + 4999]
    assert im.bins_of(pos, 5000).tolist() == [0, 0, 0, 0, 0, 0, 1, 1, 3]
    assert im.bins_of([-5000.0, -9999.0], 5000).tolist() == [-1, -1]        # C truncation, not floor
    for bad in (numpy.inf, -numpy.inf, 2.0 ** 31 * 5000):
        with pytest.raises(ValueError):
            im.bins_of([bad], 5000)


@pytest.mark.parametrize("dtype", DTYPES)
def test_value_rule(dtype):
    floor, top = im.WISH_FLOOR[dtype], im.WISH_CEILING[dtype]
    assert floor == (1e-30 if dtype == "float32" else 1e-290)
    v = [floor, numpy.nextafter(floor, 0.0), 2 * floor, 5e-324, -1.0, 0.0, numpy.nan, numpy.inf, -numpy.inf, 2.5]
    got = im.wish_from_value(v, "wish", 3.0, dtype)
    want = numpy.array([floor, 0.0, 2 * floor, 0, 0, 0, 0, 0, 0, 2.5]).astype(dtype).astype(numpy.float64)
    assert numpy.array_equal(got, want) and got[0] > 0
    # the largest distance of the dtype is one, the double after it and 1e39 are none in fp32
    got = im.wish_from_value([im.FLT_MAX, numpy.nextafter(im.FLT_MAX, numpy.inf), 1e39, top], "wish", 3.0, dtype)
    assert numpy.isfinite(got).all()
    assert got.tolist() == ([im.FLT_MAX, 0.0, 0.0, im.FLT_MAX] if dtype == "float32"
                            else [im.FLT_MAX, numpy.nextafter(im.FLT_MAX, numpy.inf), 1e39, im.DBL_MAX])
    # counts: c ** (-1 / alpha); the largest double is 1.8e-103, below the fp32 floor; 1e-120 is 1e40
    got = im.wish_from_value([8.0, 0.0, -8.0, im.DBL_MAX, 1e-120, numpy.inf], "counts", 3.0, dtype)
    assert got[0] == 0.5 and not got[[1, 2, 5]].any()
    assert (got[3] == 0.0) == (dtype == "float32") and (got[4] == 0.0) == (dtype == "float32")
    assert im.wish_from_value([27.0], "counts", 1.5, dtype)[0] == numpy.asarray(27.0 ** (-1 / 1.5), dtype=dtype)


def _loop(n, rows, cols, vals, dtype):
    """The entries rule as a Python loop over the entries."""
    w = numpy.zeros((n, n))
    for r, c, v in zip(rows, cols, vals):
        if r != c:
            w[r, c] = w[c, r] = im.wish_from_value([v], "wish", 3.0, dtype)[0]
    return w


def test_entries_rule_on_a_hand_made_list():
    rows = [0, 1, 2, 2, 3, 1, 0, 2]
    cols = [1, 0, 2, 3, 2, 3, 1, 1]
    vals = [5.0, 7.0, 9.0, 4.0, 0.0, 2.0, numpy.nan, -3.0]
    w = im.matrix_of("entries", 4, "float64", rows=rows, cols=cols, vals=vals)
    want = numpy.zeros((4, 4))
    want[1, 3] = want[3, 1] = 2.0      # (0, 1): 5, then 7 the other way round, then NaN: none
    assert numpy.array_equal(w, want)  # (2, 3): 4 loses to the later explicit 0; (2, 2) skipped; (1, 2): -3
    with pytest.raises(ValueError):
        im.matrix_of("entries", 4, "float64", rows=[0], cols=[4], vals=[1.0])
    assert not im.matrix_of("entries", 4, "float64", rows=[4], cols=[4], vals=[1.0]).any()   # a diagonal entry is skipped first


@pytest.mark.parametrize("dtype", DTYPES)
def test_last_entry_wins_three_ways(dtype):
    rng = numpy.random.default_rng(3)
    n, m = 23, 4000
    rows, cols = rng.integers(0, n, m), rng.integers(0, n, m)
    vals = im.POW2[rng.integers(0, 5, m)] * rng.choice([1.0, 1e-35, 1e39, numpy.nan], m, p=[0.7, 0.1, 0.1, 0.1])
    want = _loop(n, rows, cols, vals, dtype)
    assert numpy.array_equal(im.matrix_of("entries", n, dtype, rows=rows, cols=cols, vals=vals), want)
    assert numpy.array_equal(im.matrix_by_assignment(n, rows, cols, vals, dtype), want)
    assert numpy.array_equal(want, want.T) and not want.diagonal().any()


def test_kr_operation_order_and_nan_to_num():
    kr = numpy.array([1e200, 1e200, 2.0, numpy.nan])
    ke = numpy.array([1.0, 1e-300, 0.5, 4.0])
    # (0, 1): (1e200 * 1e200) * 1e-300 is infinite left to right (1e100 in any other order): 6 / inf = 0
    # (1, 2): 1e300 / (1e200 * 2 * 1e-300) overflows: the largest double; (2, 3): NaN bin: none
    # (0, 2): 8e200 / (1e200 * 2 * 0.5) = 8
    w = im.matrix_of("entries", 4, "float64", rows=[0, 1, 2, 0], cols=[1, 2, 3, 2], vals=[6.0, 1e300, 5.0, 8e200], kr=kr, ke=ke)
    assert w[0, 1] == 0.0 and w[1, 2] == im.DBL_MAX and w[2, 3] == 0.0 and w[0, 2] == 8.0
    # a vector shorter than the map: its missing bins are NaN
    w = im.matrix_of("entries", 4, "float64", rows=[0, 0], cols=[1, 3], vals=[4.0, 4.0], kr=[1.0, 2.0, 1.0], ke=[1.0, 2.0, 1.0])
    assert w[0, 1] == 1.0 and w[0, 3] == 0.0


def test_dense_rule_reads_the_upper_triangle():
    w = sm.integer_map(40, seed=1)
    junk = im.with_junk(w, seed=1)
    got = im.matrix_of("dense", 40, "float64", matrix=junk)
    assert numpy.array_equal(got, sm.clean_wish(junk)) and not numpy.array_equal(got, w)


def test_generated_coordinates():
    xs = im.line_coords(50, seed=2)
    w = im.matrix_of("coords", 50, "float32", xs=xs)
    t = xs[:, 0]
    assert numpy.array_equal(w, 3.0 * numpy.abs(t[:, None] - t[None, :]))
    assert im.stress_of(w, xs, "float64") < 1e-20 and im.stress_of(w, 2.0 * xs, "float64") == (w * w).sum() / 2


# ---- against the oracle ----------------------------------------------------------------------------
def _oracle_triples(n_bins, m, seed):
    rng = numpy.random.default_rng(seed)
    i, j = rng.integers(0, n_bins, m), rng.integers(0, n_bins, m)
    v = rng.integers(0, 6, m).astype(numpy.float64)
    v[rng.random(m) < 0.05] = numpy.nan
    return im.triples_of(i, j, v, seed=seed)


def test_triples_rule_equals_the_oracles_scatter_and_normalize():
    n_bins, res = 40, im.RESOLUTION
    t = _oracle_triples(n_bins, 3000, 4)
    t = t[~numpy.isnan(t[:, :2]).any(axis=1) & (t[:, :2] >= 0).all(axis=1)]    # the oracle indexes with every bin it computes
    o = _oracle.load()
    raw = o.contactmap_scatter(t, res, n_bins)
    got = im.matrix_of("triples", n_bins + 1, "float64", triples=t, resolution=res)
    # (the oracle stores the raw values, -inf as the lowest double: the value rule on both sides)
    assert numpy.array_equal(got, im.matrix_of("dense", n_bins + 1, "float64", matrix=raw)) and got.any()
    assert (raw < 0).any() and numpy.array_equal(raw, raw.T)
    rng = numpy.random.default_rng(5)
    kr, ke = rng.uniform(0.5, 2.0, n_bins), rng.uniform(0.5, 2.0, n_bins)
    kr[[3, 17]] = numpy.nan
    norm = o.contactmap_normalize(raw, kr, ke)
    got = im.matrix_of("triples", n_bins + 1, "float64", triples=t, resolution=res, kr=kr, ke=ke)
    assert numpy.array_equal(got, im.matrix_of("dense", n_bins + 1, "float64", matrix=norm))
    assert not got[3].any() and got[5].any() and not numpy.array_equal(norm, raw)


def test_counts_rule_equals_the_oracles():
    c = numpy.random.default_rng(6).poisson(3.0, (30, 30)).astype(numpy.float64)
    c = c + c.T
    c[2, 9] = c[9, 2] = numpy.inf
    want = _oracle.load().counts_to_wish(c, 3.0)
    got = im.matrix_of("dense", 30, "float64", kind="counts", alpha=3.0, matrix=c)
    assert got[2, 9] == 0.0 and numpy.abs(got - want).max() <= 4 * 2.0 ** -53 * want.max()


# ---- the exactness preconditions of the GPU cases -------------------------------------------------
def _exact(w, n):
    return all(im.sixteenths_exact(w, x) for x in im.rhs(n))


@pytest.mark.parametrize("case", im.CASES + (("float32", 300),), ids=_ids)
def test_dense_cm_and_coords_cases_are_exact(case):
    dtype, n = case
    clean, junk = im.dense_case(n)
    w = im.matrix_of("dense", n, dtype, matrix=junk)
    assert _exact(clean, n) and _exact(w, n)
    assert set(numpy.unique(w)) == set(im.POW2) and 0.05 < (w != clean).mean() < 0.15
    ints = im.dense_case(n, "integer")[0]
    assert all(sm.largest_partial_sum(ints, x) < sm.MAX_EXACT for x in im.rhs(n))
    xs = im.matrix_of("coords", n, dtype, xs=im.coords_case(n))
    assert all(sm.largest_partial_sum(xs, x) < sm.MAX_EXACT for x in im.rhs(n))
    assert numpy.array_equal(xs, numpy.round(xs))


@pytest.mark.parametrize("with_kr", [False, True])
@pytest.mark.parametrize("band", [None, im.BAND])
@pytest.mark.parametrize("case", im.CASES + (("float32", 300),), ids=_ids)
def test_entry_and_triple_cases_are_exact(case, band, with_kr):
    dtype, n = case
    for huge in (True, False):
        rows, cols, vals, kr, ke = im.sparse_case(n, band, with_kr, huge)
        w = im.matrix_of("entries", n, dtype, rows=rows, cols=cols, vals=vals, kr=kr, ke=ke)
        t = im.triples_case(n, band, with_kr, huge)[0]
        wt = im.matrix_of("triples", n, dtype, triples=t, resolution=im.RESOLUTION, kr=kr, ke=ke)
        assert _exact(w, n) and _exact(wt, n)
        cells = set(numpy.unique(w)) | set(numpy.unique(wt))
        if huge:
            # +inf: nothing as an entry without KR, the largest double from triples and from a KR
            # quotient -- 1.8e308 (or an eighth of it) in fp64, no constraint in fp32
            hot = (wt > 1e150).sum()
            assert hot == (0 if dtype == "float32" else (6 if not with_kr else hot)) and (with_kr or not (w > 1e150).any())
            assert hot > 0 or dtype == "float32"
        else:
            assert numpy.array_equal(w, wt) and cells == set(im.POW2)
    # the last of a pair's entries wins, an explicit 0 over an earlier distance too
    lo, hi, k = im.last_of_each_pair(n, rows, cols)
    assert 0.2 < 1.0 - lo.size / float((rows != cols).sum()) < 0.5               # pairs named again
    _, _, k_rev = im.last_of_each_pair(n, rows[::-1], cols[::-1])                # (the FIRST entry of each pair)
    assert ((vals[::-1][k_rev] > 0) & (vals[k] == 0)).sum() > 10
    assert (rows == cols).any() and (rows > cols).any() and (rows < cols).any()
    if with_kr:
        assert numpy.isnan(kr).any() and numpy.isnan(ke).any() and not w[numpy.isnan(kr)].any()
        assert len(set(numpy.unique(ke[numpy.isfinite(ke)]))) == 7


def test_triples_cases_sit_anywhere_in_their_bins():
    t = im.triples_case(700, None, False)[0]
    res = im.RESOLUTION
    p = t[:, :2].ravel()
    assert numpy.isnan(p).any() and ((p > -res) & (p < 0)).any() and (p % res == res - 1).any()
    assert (p % 1 != 0).any() and (p % res == 0).any()
    assert numpy.isnan(t[:, 2]).any() and (t[:, 2] == numpy.inf).any() and (t[:, 2] == -numpy.inf).any()
    assert not numpy.asfortranarray(t).flags.c_contiguous


@pytest.mark.parametrize("dtype", DTYPES)
def test_seam_case(dtype):
    rows, cols, vals, marks = im.seam_case()
    n, c = im.SEAM_BINS, im.SEAM_CHUNK
    assert rows.size == c + 100000 and marks["final of chunk 0"][0] == c - 1 and marks["first of chunk 1"][0] == c
    w = im.matrix_by_assignment(n, rows, cols, vals, dtype)
    assert numpy.array_equal(w, im.matrix_of("entries", n, dtype, rows=rows, cols=cols, vals=vals))
    assert _exact(w, n)
    lo, hi = numpy.minimum(rows, cols), numpy.maximum(rows, cols)
    key0, key1 = numpy.unique((lo * n + hi)[:c][lo[:c] != hi[:c]]), numpy.unique((lo * n + hi)[c:][lo[c:] != hi[c:]])
    both = numpy.intersect1d(key0, key1)
    only0 = numpy.setdiff1d(key0, key1)
    assert both.size > 50000 and only0.size > 100000
    assert (w.reshape(-1)[only0] > 0).sum() > 0.5 * only0.size                    # they survive chunk 1
    # among the pairs of both chunks, chunk 1's value differs from chunk 0's last in many
    w0 = im.matrix_by_assignment(n, rows[:c], cols[:c], vals[:c], dtype)
    assert (w.reshape(-1)[both] != w0.reshape(-1)[both]).sum() > 0.5 * both.size
    assert (w[0, 1], w[0, 2], w[0, 3], w[1, 2]) == (2.0, 0.25, 0.0, 0.5) and w0[0, 3] == 1.0 and w0[0, 2] == 0.0


@pytest.mark.parametrize("dtype", DTYPES)
def test_several_maps_case(dtype):
    total, offsets, maps, tiles = im.many_case(dtype)
    vw = 512 if dtype == "float32" else 128
    assert total == offsets[-1] + maps[-1].shape[0] and all(a % vw == 0 for a in offsets)
    key = tiles[1].astype(numpy.int64) * 64 + tiles[0]
    assert (numpy.diff(key) > 0).all() and (tiles[0] <= tiles[1]).all()          # device order, I <= J
    starts = numpy.asarray(offsets) // vw
    assert (numpy.searchsorted(starts, tiles[0], side="right") == numpy.searchsorted(starts, tiles[1], side="right")).all()
    w = im.block_diagonal(total, zip(offsets, maps))
    s = im.weight_sums_of(w, 2)
    assert numpy.array_equal(16 * s, numpy.round(16 * s)) and not w[700 if dtype == "float32" else 300:offsets[1]].any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_several_maps_composites_are_exact(dtype):
    """The matrices test_several_maps_block_setters goes through: the junk maps, map 1 written
    again (seed 99), the smaller block (seed 5) at map 0's first bin."""
    total, offsets, maps, _ = im.many_case(dtype)
    vw = 512 if dtype == "float32" else 128
    cleaned = [im.matrix_of("dense", m.shape[0], dtype, matrix=im.with_junk(m, seed=off)) for m, off in zip(maps, offsets)]
    other, small = im.pow2_map(maps[1].shape[0], seed=99), im.pow2_map(200, seed=5)
    assert not numpy.array_equal(other, cleaned[1])
    w = im.block_diagonal(total, zip(offsets, [cleaned[0], other, cleaned[2]]))
    steps = [im.block_diagonal(total, zip(offsets, cleaned)), w.copy()]
    edge = -(-200 // vw) * vw
    w[:edge, :edge] = 0.0
    w[:200, :200] = small
    steps.append(w)
    x = sm.integer_rhs(total, seed=1)
    assert all(im.sixteenths_exact(m, x) for m in steps)
    assert steps[2][:edge, :edge].sum() < steps[1][:edge, :edge].sum() and numpy.array_equal(steps[2][edge:], steps[1][edge:])


@pytest.mark.parametrize("dtype,n,vw", [("float32", 1537, 512), ("float64", 300, 128)])
def test_block_at_an_offset_composite_is_exact(dtype, n, vw):
    off = (n - 1) // vw * vw
    w = im.dense_case(n)[0].copy()
    w[off:, off:] = im.pow2_map(n - off, seed=17)
    assert 0 < off < n and _exact(w, n) and numpy.array_equal(w, w.T)


@pytest.mark.parametrize("dtype,n", im.FLOAT_CASES)
def test_float_case(dtype, n):
    t, kr, ke = im.float_case(n, seed=n)
    assert numpy.isinf(t[:, 2]).sum() == 1 and numpy.isnan(kr).any() and numpy.isnan(ke).any()
    i, j = im.bins_of(t[:, 0], im.RESOLUTION), im.bins_of(t[:, 1], im.RESOLUTION)
    assert max(i.max(), j.max()) < n - 1 and (i < j).all()                       # the padding bin is not named
    k = int(numpy.flatnonzero(numpy.isinf(t[:, 2]))[0])
    quotient = im.matrix_of("triples", n, "float64", triples=t[k:k + 1], resolution=im.RESOLUTION, kr=kr, ke=ke)
    assert quotient.max() == im.DBL_MAX                                           # the overflowing quotient
    w = im.matrix_of("triples", n, dtype, kind="counts", triples=t[k:k + 1], resolution=im.RESOLUTION, kr=kr, ke=ke)
    assert (w.max() > 0) == (dtype == "float64") and w.max() < 1e-100
