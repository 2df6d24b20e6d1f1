"""GPU: every route a wish-distance map takes into the solver's units -- bb_solver_set_wish_dense
[_block], _from_cm [_block], _sparse, _triples (with bb_triples_tiles), _from_coords, and the
row-owner copy made of the units (units_to_full_kernel) -- against the numpy model of
tests/_input_model.py, cell for cell, on the three unit layouts.

A cell cannot be read back, so a route is probed by its `signature`: bb_solver_degrees (exact
counts), bb_solver_weight_sums at q = 2 (float64) and bb_solver_matvec_sq of six integer vectors.
On the maps used here -- wish distances in {0, 1/4, 1/2, 1, 2}, right-hand sides in [-2, 2] --
every term and every partial sum is exact in float32 and float64 whatever the order
(tests/test_input_model_cpu.py asserts that for every case), so the device must return the
model's bits: a wrong value at (i, j) changes y_i by err * x_j, a displaced cell the sums of its
old and its new bin.  Where a map's weights are not powers of two (integer maps, generated
coordinates: 1/9) the weight sums are held to their rounding bound, (n + 16) 2^-53 s_i, instead.

Float maps (B) are held to the allowances the suite already has: SPEC 4's 1e-12 for the device's
pow in fp64 and the 2^-21 of tests/test_gpu_score.py in fp32."""
import numpy
import pytest

import blueberry_amd as bb
from blueberry_amd.solver import DeviceTriples, GroupEngine, HipEngine, layout_info, tiles_from_entries
from tests import _input_model as im
from tests import _spectral_model as sm
from tests.test_gpu_parity import solver_path                     # noqa: F401

pytestmark = pytest.mark.gpu

ALPHA = 3.0
BANDED = tuple(c for c in im.CASES if c[1] >= 1300)       # sizes at which a band leaves tiles out
_ids = lambda c: "%s-%d" % c                              # noqa: E731


# ---- probes ---------------------------------------------------------------------------------------
def signature(e, n, several=False):
    """(degrees, weight sums at q = 2[, two matvec_sq blocks])."""
    e.set_weight_power(2)
    out = (e.degrees(), e.weight_sums())
    return out if several else out + tuple(e.matvec_sq(x) for x in im.rhs(n))


def _same(got, want, what):
    bad = numpy.argwhere(got != want)
    assert bad.size == 0, (what, "%d wrong, first at %s: %r != %r"
                           % (len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])]))


def check(sig, w, n, what, exact_sums=True):
    """The signature `sig` (an engine's, or the sum of the ranks') is the model matrix w's."""
    _same(sig[0], im.degrees_of(w), (what, "degrees"))
    want = im.weight_sums_of(w, 2)
    if exact_sums:
        _same(sig[1], want, (what, "weight sums"))
    else:
        assert (numpy.abs(sig[1] - want) <= im.weight_sum_bound(w, 2, 0.0)).all(), (what, "weight sums")
    # a cell of 1.8e308 (an infinite count in fp64) squares to +inf: its two rows are left out
    # of the product, and so are the 8 rows on either side of them -- the sweep folds the sums
    # of neighbouring rows in one reduction, where inf * 0 turns one more row NaN (seen on the
    # 2 x 512 units, up to 3 rows away); degrees and weight sums (1 / inf = 0) hold everywhere
    cool = numpy.ones(n, dtype=bool)
    for h in numpy.flatnonzero((w > 1e150).any(axis=1)):
        cool[max(0, h - 8):h + 9] = False
    assert cool.sum() >= n - 17 * 6
    fin = numpy.where(w < 1e150, w, 0.0)
    for got, x in zip(sig[2:], im.rhs(n)):
        _same(got[cool], im.matvec_sq_of(fin, x)[cool], (what, "matvec_sq"))


def _engine(n, dtype, tiles=None, **kw):
    e = HipEngine(n, dtype, tiles=tiles, **kw)
    lay = e.layout()
    assert (lay["vw"], lay["rows_per_unit"]) == im.LAYOUTS[(dtype, n)]
    return e


def _strided(m):
    """m as a slice of a wider array: ld > n."""
    n = m.shape[0]
    wide = numpy.full((n, n + 37), numpy.nan)
    wide[:, 5:5 + n] = m
    view = wide[:, 5:5 + n]
    assert view.strides == (8 * (n + 37), 8)
    return view


def _band_tiles(n, dtype, rows, cols):
    tiles = tiles_from_entries(n, rows, cols, dtype)
    assert len(tiles[0]) < layout_info(n, dtype)["n_tiles"]           # some tiles are absent
    return tiles


# ---- the instrument: weight sums on the dense host route ----------------------------------------
@pytest.mark.parametrize("which", ["pow2", "integer"])
@pytest.mark.parametrize("case", im.CASES, ids=_ids)
def test_weight_sums_equal_the_model_on_the_dense_host_route(case, which):
    """bb_solver_weight_sums (and degrees) on set_wish_dense of a clean C-contiguous matrix:
    bit for bit on the power-of-two map, within the rounding bound on the integer one."""
    dtype, n = case
    w = im.dense_case(n, which)[0]
    e = _engine(n, dtype)
    try:
        e.set_wish_dense(w, "wish", ALPHA)
        check(signature(e, n), w, n, (case, which), exact_sums=which == "pow2")
    finally:
        e.close()


# ---- A. every route against the model, bit for bit ---------------------------------------------
@pytest.mark.parametrize("form", ["contiguous", "strided"])
@pytest.mark.parametrize("case", im.CASES, ids=_ids)
def test_set_wish_dense(case, form):
    """convert_units_kernel behind hipMemcpy2DAsync: a non-zero diagonal, junk in a tenth of the
    pairs and in the whole lower triangle; C-contiguous and as a slice of a wider array."""
    dtype, n = case
    junk = im.dense_case(n)[1]
    w = im.matrix_of("dense", n, dtype, matrix=junk)
    e = _engine(n, dtype)
    try:
        e.set_wish_dense(junk if form == "contiguous" else _strided(junk), "wish", ALPHA)
        check(signature(e, n), w, n, (case, form))
    finally:
        e.close()


@pytest.mark.parametrize("case", im.CASES, ids=_ids)
def test_set_wish_from_cm(case):
    """pack_units_from_matrix_kernel from a resident ContactMap holding the junk matrix, which
    the route leaves as it was."""
    dtype, n = case
    junk = im.dense_case(n)[1]
    w = im.matrix_of("dense", n, dtype, matrix=junk)
    dev = bb.ContactMap.from_matrix(junk)._resident()
    e = _engine(n, dtype)
    try:
        e.set_wish_from_cm(dev, "wish", ALPHA)
        check(signature(e, n), w, n, case)
        assert numpy.array_equal(dev.to_host(), junk, equal_nan=True)
    finally:
        e.close()
        dev.close()


SPARSE = ([(c, None, kr) for c in im.CASES for kr in (False, True)]
          + [(c, im.BAND, kr) for c in BANDED for kr in (False, True)])


@pytest.mark.parametrize("case,band,with_kr", SPARSE,
                         ids=["%s-%d-%s-%s" % (c + ("band" if b else "dense", "kr" if k else "raw")) for c, b, k in SPARSE])
def test_set_wish_sparse(case, band, with_kr):
    """scatter_entries_kernel from host entries: both orientations, 30 % of the pairs named
    again in random order (the last wins, an explicit 0 included), diagonal entries, +inf
    values, with and without power-of-two KR vectors whose NaNs drop their bins' pairs."""
    dtype, n = case
    rows, cols, vals, kr, ke = im.sparse_case(n, band, with_kr)
    w = im.matrix_of("entries", n, dtype, rows=rows, cols=cols, vals=vals, kr=kr, ke=ke)
    e = _engine(n, dtype, tiles=_band_tiles(n, dtype, rows, cols) if band else None)
    try:
        e.set_wish_sparse(rows, cols, vals, "wish", ALPHA, kr, ke)
        check(signature(e, n), w, n, (case, band, with_kr))
    finally:
        e.close()


TRIPLES = ([(c, None, kr, order) for c in im.CASES for kr in (False, True) for order in "CF"]
           + [(c, im.BAND, kr, order) for c in BANDED for kr, order in ((False, "F"), (True, "C"))])


@pytest.mark.parametrize("case,band,with_kr,order", TRIPLES,
                         ids=["%s-%d-%s-%s-%s" % (c + ("band" if b else "dense", "kr" if k else "raw", o))
                              for c, b, k, o in TRIPLES])
def test_set_wish_triples(case, band, with_kr, order):
    """The same kernel from resident triples (entry_pair's nan_to_num and truncation): positions
    anywhere inside their bin, in (-res, 0) and NaN for bin 0; NaN, +inf and -inf counts; row-
    and column-major.  bb_triples_tiles names the tiles of the model's bins.  A position of +inf
    and a bin outside the map are refused and leave the engine usable."""
    dtype, n = case
    t, kr, ke = im.triples_case(n, band, with_kr)
    w = im.matrix_of("triples", n, dtype, triples=t, resolution=im.RESOLUTION, kr=kr, ke=ke)
    i, j = im.bins_of(t[:, 0], im.RESOLUTION), im.bins_of(t[:, 1], im.RESOLUTION)
    want_tiles = tiles_from_entries(n, i[i != j], j[i != j], dtype)
    dev = DeviceTriples(numpy.asfortranarray(t) if order == "F" else numpy.ascontiguousarray(t), im.RESOLUTION, 0)
    got_tiles = dev.tiles(n, dtype)
    assert set(zip(*got_tiles)) == set(zip(*want_tiles))
    e = _engine(n, dtype, tiles=_band_tiles(n, dtype, i, j) if band else None)
    try:
        for pos_i, pos_j in ((numpy.inf, 0.0), (float(n * im.RESOLUTION), 0.0)):
            bad = DeviceTriples(numpy.array([[0.0, float(im.RESOLUTION), 1.0], [pos_i, pos_j, 1.0]]),
                                im.RESOLUTION, 0)
            with pytest.raises(ValueError):
                e.set_wish_triples(bad, "wish", ALPHA)
            bad.close()
        e.set_wish_triples(dev, "wish", ALPHA, kr, ke)
        check(signature(e, n), w, n, (case, band, with_kr, order))
    finally:
        e.close()
        dev.close()


@pytest.mark.parametrize("case", im.CASES, ids=_ids)
def test_set_wish_from_coords(case):
    """gen_units_kernel on x*_i = t_i (1, 2, 2): distances 3 |t_i - t_j|, coincident bins none."""
    dtype, n = case
    xs = im.coords_case(n)
    w = im.matrix_of("coords", n, dtype, xs=xs)
    assert set(numpy.unique(w)) == {0.0, 3.0, 6.0, 9.0}
    e = _engine(n, dtype)
    try:
        e.set_wish_from_coords(xs)
        check(signature(e, n), w, n, case, exact_sums=False)
    finally:
        e.close()


# ---- rank shares -----------------------------------------------------------------------------------
def _fill(e, route, n, dtype, huge=True):
    """Fill engine `e` by `route` from the shared cases; returns (model matrix, what to close)."""
    if route in ("dense", "cm", "dense_block", "cm_block"):
        junk = im.dense_case(n)[1]
        w = im.matrix_of("dense", n, dtype, matrix=junk)
        if route == "dense":
            e.set_wish_dense(_strided(junk), "wish", ALPHA)
            return w, None
        if route.endswith("_block"):                   # the whole map as one block at bin 0
            _put(e, route, junk, 0)
            return w, None
        dev = bb.ContactMap.from_matrix(junk)._resident()
        e.set_wish_from_cm(dev, "wish", ALPHA)
        return w, dev
    if route == "sparse":
        rows, cols, vals, kr, ke = im.sparse_case(n, None, True, huge)
        e.set_wish_sparse(rows, cols, vals, "wish", ALPHA, kr, ke)
        return im.matrix_of("entries", n, dtype, rows=rows, cols=cols, vals=vals, kr=kr, ke=ke), None
    if route == "triples":
        t, kr, ke = im.triples_case(n, None, True, huge)
        dev = DeviceTriples(numpy.asfortranarray(t), im.RESOLUTION, 0)
        e.set_wish_triples(dev, "wish", ALPHA, kr, ke)
        return im.matrix_of("triples", n, dtype, triples=t, resolution=im.RESOLUTION, kr=kr, ke=ke), dev
    assert route == "coords"
    e.set_wish_from_coords(im.coords_case(n))
    return im.matrix_of("coords", n, dtype, xs=im.coords_case(n)), None


@pytest.mark.parametrize("route", ["cm", "sparse", "triples"])
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("case", [("float32", 300), ("float32", 1537), ("float64", 1300), ("float64", 4097)], ids=_ids)
def test_rank_shares_add_up_to_the_model(case, world, route):
    """Every rank packs its own units (the routes' u_begin / u_end filters): the ranks' degrees,
    weight sums and products add up to the model's exactly.  300 bins in fp32 are one tile of 128
    units whose rows from 300 on are padding: the last of three ranks owns no pair."""
    dtype, n = case
    total, w = None, None
    for rank in range(world):
        e = _engine(n, dtype, rank=rank, world=world)
        try:
            w, dev = _fill(e, route, n, dtype)
            sig = signature(e, n)
            if dev is not None:
                dev.close()
        finally:
            e.close()
        total = sig if total is None else tuple(a + b for a, b in zip(total, sig))
    check(total, w, n, (case, world, route))
    if case == ("float32", 300) and world == 3:
        assert not sig[0].any() and not sig[1].any()


def test_group_of_three_members_on_one_device():
    """GroupEngine(devices=[0, 0, 0]): set_wish_resident and set_wish_triples reach every member."""
    dtype, n = "float32", 1537
    junk = im.dense_case(n)[1]
    t, kr, ke = im.triples_case(n, None, True)
    cm = bb.ContactMap.from_matrix(junk)
    dev = DeviceTriples(t, im.RESOLUTION, 0)
    g = GroupEngine(n, dtype, devices=[0, 0, 0])
    try:
        g.set_wish_resident(cm, "wish", ALPHA)
        check(signature(g, n), im.matrix_of("dense", n, dtype, matrix=junk), n, "group, resident")
        g.set_wish_triples(dev, "wish", ALPHA, kr, ke)
        check(signature(g, n), im.matrix_of("triples", n, dtype, triples=t, resolution=im.RESOLUTION, kr=kr, ke=ke),
              n, "group, triples")
    finally:
        g.close()
        dev.close()


# ---- the chunk seam of set_wish_sparse -------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_set_wish_sparse_across_its_chunk_seam(dtype):
    """2^22 + 100,000 entries: the second chunk's clear / mark / store phases run on top of the
    first chunk's cells.  A pair of both chunks keeps chunk 1's entry (an explicit 0 included),
    the final entry of chunk 0 and the first of chunk 1 count, a pair of chunk 0 alone survives."""
    n = im.SEAM_BINS
    rows, cols, vals, marks = im.seam_case()
    assert rows.size > im.SEAM_CHUNK
    w = im.matrix_by_assignment(n, rows, cols, vals, dtype)
    assert (w[0, 1], w[0, 2], w[0, 3], w[1, 2]) == (2.0, 0.25, 0.0, 0.5)
    e = _engine(n, dtype)
    try:
        e.set_wish_sparse(rows, cols, vals, "wish", ALPHA)
        check(signature(e, n), w, n, ("seam", dtype))
    finally:
        e.close()


# ---- several maps in one solver --------------------------------------------------------------------
def _put(e, setter, m, off):
    if setter == "dense_block":
        e.set_wish_dense_block(_strided(m), off, "wish", ALPHA)
        return
    dev = bb.ContactMap.from_matrix(m)._resident()
    try:
        e.set_wish_from_cm_block(dev, off, "wish", ALPHA)
    finally:
        dev.close()


@pytest.mark.parametrize("setter", ["dense_block", "cm_block"])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_several_maps_block_setters(dtype, setter):
    """Three maps on their own dense triangles, filled one by one (`off` > 0 of
    set_wish_dense_t and of pack_units_from_matrix_kernel): the block-diagonal model, degree 0 in
    the padding bins; overwriting map 1 leaves maps 0 and 2 bit for bit; a smaller block written
    at map 0's first bin clears the rest of the tiles it touches and no other tile."""
    total, offsets, maps, tiles = im.many_case(dtype)
    vw = layout_info(total, dtype)["vw"]
    assert vw == (512 if dtype == "float32" else 128)
    e = HipEngine(total, dtype, tiles=tiles)
    try:
        e.set_maps(list(offsets) + [total], [1.0] * len(maps))
        junk = [im.with_junk(m, seed=off) for m, off in zip(maps, offsets)]
        maps = [im.matrix_of("dense", m.shape[0], dtype, matrix=m) for m in junk]
        for m, off in zip(junk, offsets):
            _put(e, setter, m, off)
        w = im.block_diagonal(total, zip(offsets, maps))
        first = signature(e, total, several=True)
        check(first, w, total, (dtype, setter, "three maps"))
        for a, b in zip(offsets[1:], (off + m.shape[0] for off, m in zip(offsets, maps))):
            assert not first[0][b:a].any()                               # padding between the maps
        other = im.pow2_map(maps[1].shape[0], seed=99)
        _put(e, setter, other, offsets[1])
        w = im.block_diagonal(total, zip(offsets, [maps[0], other, maps[2]]))
        second = signature(e, total, several=True)
        check(second, w, total, (dtype, setter, "map 1 again"))
        for q in (0, 2):
            rng = slice(offsets[q], offsets[q] + maps[q].shape[0])
            assert numpy.array_equal(first[0][rng], second[0][rng]) and numpy.array_equal(first[1][rng], second[1][rng])
        n_sub = 200
        small = im.pow2_map(n_sub, seed=5)
        _put(e, setter, small, 0)
        edge = -(-n_sub // vw) * vw                    # the tiles with a column below n_sub
        w[:edge, :edge] = 0.0
        w[:n_sub, :n_sub] = small
        check(signature(e, total, several=True), w, total, (dtype, setter, "a smaller block"))
    finally:
        e.close()


@pytest.mark.parametrize("setter", ["dense_block", "cm_block"])
@pytest.mark.parametrize("dtype,n", [("float32", 1537), ("float64", 300)])
def test_block_at_an_offset_leaves_the_tiles_above_it(dtype, n, setter):
    """A one-map dense solver: a block written at the last tile edge replaces the tiles from
    that edge on; the tiles that join earlier rows with its columns keep what they hold."""
    vw = layout_info(n, dtype)["vw"]
    off = (n - 1) // vw * vw
    w = im.dense_case(n)[0].copy()
    block = im.pow2_map(n - off, seed=17)
    e = _engine(n, dtype)
    try:
        e.set_wish_dense(w, "wish", ALPHA)
        _put(e, setter, block, off)
        w[off:, off:] = block
        check(signature(e, n), w, n, (dtype, n, setter))
    finally:
        e.close()


# ---- B. float maps: the routes agree bit for bit --------------------------------------------------
@pytest.mark.parametrize("dtype,n", im.FLOAT_CASES)
def test_float_map_four_routes_one_signature(dtype, n):
    """A Hi-C-like count map with KR vectors that hold NaNs and one quotient that overflows to
    the largest double, kind='counts', alpha 3: raw triples + KR, binned entries + KR, the
    normalised resident ContactMap and its host matrix leave the same units -- the four
    signatures are equal bit for bit (include/blueberry_hip.h: "exactly what the dense
    ContactMap path gives").  Against the model: degrees exact, weight sums at q = 1 within
    (extra + (n + 16) 2^-53) s_i, extra = 1e-12 (fp64) / 2^-21 (fp32).  The ContactMap's last bin
    is its padding bin, which no triple names (a KR vector has no entry for it)."""
    t, kr, ke = im.float_case(n, seed=n)
    w = im.matrix_of("triples", n, dtype, kind="counts", alpha=ALPHA, triples=t, resolution=im.RESOLUTION, kr=kr, ke=ke)
    i, j = im.bins_of(t[:, 0], im.RESOLUTION), im.bins_of(t[:, 1], im.RESOLUTION)
    cm = bb.ContactMap.from_triples(t, im.RESOLUTION, n - 1, KRnorm=kr, KRexpected=ke)
    cm.normalize()
    host = cm.to_host()
    dev_cm = cm._resident()
    assert host.max() == im.DBL_MAX                                      # the overflowing quotient
    dev_t = DeviceTriples(t, im.RESOLUTION, 0)
    fills = {"triples": lambda e: e.set_wish_triples(dev_t, "counts", ALPHA, kr, ke),
             "sparse": lambda e: e.set_wish_sparse(i, j, t[:, 2], "counts", ALPHA, kr, ke),
             "cm": lambda e: e.set_wish_from_cm(dev_cm, "counts", ALPHA),
             "dense": lambda e: e.set_wish_dense(host, "counts", ALPHA)}
    sigs = {}
    try:
        for name, fill in fills.items():
            e = _engine(n, dtype)
            try:
                fill(e)
                sigs[name] = signature(e, n)
                e.set_weight_power(1)
                sigs[name] += (e.weight_sums(),)
            finally:
                e.close()
    finally:
        dev_t.close()
        dev_cm.close()
    for name in ("sparse", "cm", "dense"):
        for a, b in zip(sigs["triples"], sigs[name]):
            assert numpy.array_equal(a, b, equal_nan=True), (dtype, n, name)
    _same(sigs["triples"][0], im.degrees_of(w), "degrees")
    bound = im.weight_sum_bound(w, 1, 1e-12 if dtype == "float64" else 2.0 ** -21)
    err = numpy.abs(sigs["triples"][4] - im.weight_sums_of(w, 1))
    ratio = float((err / numpy.where(bound > 0, bound, 1.0)).max())
    print("float map %s N=%d: %d pairs, largest |weight sum - model| / bound = %.3g"
          % (dtype, n, int(im.degrees_of(w).sum()) // 2, ratio))
    assert ((bound > 0) | (err == 0)).all() and (err <= bound).all()


# ---- C. the row-owner copy ----------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["dense", "cm", "sparse", "triples", "coords", "dense_block", "cm_block"])
@pytest.mark.parametrize("case", im.SMALL, ids=_ids)
def test_two_iterations_equal_the_dense_route(case, route, solver_path):
    """Up to 4,096 bins on one rank the iterations read a copy of both triangles made from the
    units (units_to_full_kernel, refresh_full).  The engine first holds another map -- every
    pair at distance 1 -- and its stress at the start is the model's for THAT map; then the route
    fills it, and two iterations equal bit for bit those of an engine filled by set_wish_dense
    from the model's matrix, whose first stress is the model's for the route's map (1e-12 / 1e-5,
    SPEC 4).  A copy that is not rebuilt cannot give both stresses, whatever it holds.  The
    block setters write the whole map at bin 0 (a solver of several maps has no such copy:
    bb_solver_set_maps switches to the unit sweep).  On the unit sweep too."""
    dtype, n = case
    x0, lr = sm.start_block(n, seed=n), 1.0 / (2 * n)
    ones = numpy.ones((n, n)) - numpy.eye(n)
    e, ref = _engine(n, dtype), _engine(n, dtype)
    try:
        assert (e.iteration_path()[0] == "row_owner") == (solver_path == "row_owner")
        e.set_wish_dense(ones, "wish", ALPHA)
        e.set_coords(x0)
        e.iterate(1, lr)
        assert abs(e.stress_history()[-1] / im.stress_of(ones, x0, dtype) - 1) < sm.TOL_T[dtype]
        w, dev = _fill(e, route, n, dtype, huge=False)
        if dev is not None:
            dev.close()
        assert abs(im.stress_of(w, x0, dtype) / im.stress_of(ones, x0, dtype) - 1) > 0.01
        ref.set_wish_dense(w, "wish", ALPHA)
        for eng in (e, ref):
            eng.set_coords(x0)
            eng.iterate(2, lr)
        h = ref.stress_history()
        assert h.shape == (2,) and abs(h[0] / im.stress_of(w, x0, dtype) - 1) < sm.TOL_T[dtype]
        assert numpy.array_equal(e.get_coords(), ref.get_coords())
        assert numpy.array_equal(e.stress_history()[-2:], h)
    finally:
        e.close()
        ref.close()


# ---- D. the value rule at its edges --------------------------------------------------------------
def _edge_values(dtype):
    """[(kind, value)]: each goes to a pair of its own, (2k, 2k + 1), so every sum has one term."""
    floor = im.WISH_FLOOR[dtype]
    wish = [floor, numpy.nextafter(floor, 0.0), 2.0 * floor, 5e-324, 1.0, im.FLT_MAX,
            numpy.nextafter(im.FLT_MAX, numpy.inf), 1e39]
    # FLT_MAX^-3 (1 + 1e-9): the count whose distance is the largest float32 -- 3e-10 below it
    # in float64, well inside the last float32 step and the allowance for pow
    counts = [im.DBL_MAX, im.FLT_MAX ** -3.0 * (1.0 + 1e-9), 1e-120, 8.0]
    return [("wish", float(v)) for v in wish], [("counts", float(v)) for v in counts]


@pytest.mark.parametrize("route", ["dense", "cm", "sparse", "triples", "dense_block", "cm_block"])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_value_rule_at_its_edges(dtype, route):
    """SPEC 2.1 through degrees and weight sums at q = 1: a distance at the wish floor is a
    constraint, one ulp below it and the smallest subnormal are none; the largest double as a
    count (1.8e-103) is a constraint in fp64 and none in fp32; the largest float32 is a
    constraint; a FINITE distance that float32 cannot hold (1e39, the double after FLT_MAX, the
    count 1e-120) is no constraint in fp32 -- never an infinite distance -- and an ordinary
    constraint in fp64."""
    for values in _edge_values(dtype):
        kind = values[0][0]
        v = numpy.array([x for _, x in values])
        n = 2 * v.size + 3
        lo = 2 * numpy.arange(v.size)
        m = numpy.zeros((n, n))
        m[lo, lo + 1] = m[lo + 1, lo] = v
        w = im.matrix_of("dense", n, dtype, kind=kind, alpha=ALPHA, matrix=m)
        assert numpy.isfinite(w).all()
        e = HipEngine(n, dtype)
        dev = None
        try:
            if route == "dense":
                e.set_wish_dense(m, kind, ALPHA)
            elif route == "cm":
                dev = bb.ContactMap.from_matrix(m)._resident()
                e.set_wish_from_cm(dev, kind, ALPHA)
            elif route == "sparse":
                e.set_wish_sparse(lo + 1, lo, v, kind, ALPHA)
            elif route == "dense_block":
                e.set_wish_dense_block(m, 0, kind, ALPHA)
            elif route == "cm_block":
                dev = bb.ContactMap.from_matrix(m)._resident()
                e.set_wish_from_cm_block(dev, 0, kind, ALPHA)
            else:
                dev = DeviceTriples(numpy.column_stack([lo * float(im.RESOLUTION), (lo + 1.0) * im.RESOLUTION, v]),
                                    im.RESOLUTION, 0)
                e.set_wish_triples(dev, kind, ALPHA)
            e.set_weight_power(1)
            deg, sums = e.degrees(), e.weight_sums()
        finally:
            e.close()
            if dev is not None:
                dev.close()
        print("value rule %s %s %s: constraints %s" % (dtype, route, kind, deg[lo].tolist()))
        _same(deg, im.degrees_of(w), (dtype, route, kind, "degrees"))
        assert numpy.isfinite(sums).all()
        want = im.weight_sums_of(w, 1)
        if kind == "wish":
            _same(sums, want, (dtype, route, kind, "weight sums"))
        else:
            bound = im.weight_sum_bound(w, 1, 1e-12 if dtype == "float64" else 2.0 ** -21)
            assert (numpy.abs(sums - want) <= bound).all(), (dtype, route, kind)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_value_rule_at_its_edges_from_coordinates(dtype):
    """gen_units_kernel reaches the flush without wish_from_value.  Points on the x axis (the
    other two coordinates 0: every distance is sqrt(dx * dx), one rounding each, the same in
    numpy) at 0, `low`, 1, FLT_MAX, 1e39 and 1e200.  low is the fp32 wish floor in fp32 -- a
    constraint -- and 1e-150 in fp64: the square of a separation near the fp64 floor, 1e-580, is
    0 in float64, so no generated distance comes near that floor.  A separation of FLT_MAX is a
    constraint, 1e39 and 1e39 - FLT_MAX are none in fp32, and 1e200 -- whose square is +inf in
    float64 -- is none in either dtype."""
    low = im.WISH_FLOOR[dtype] if dtype == "float32" else 1e-150
    xs = numpy.zeros((6, 3))
    xs[:, 0] = [0.0, low, 1.0, im.FLT_MAX, 1e39, 1e200]
    with numpy.errstate(over="ignore"):
        w = im.matrix_of("coords", 6, dtype, xs=xs)
    assert numpy.isfinite(w).all() and abs(w[0, 1] / low - 1) < 1e-6 and w[0, 3] == im.FLT_MAX
    assert not w[5].any() and (w[0, 4] > 0) == (dtype == "float64") and (w[3, 4] > 0) == (dtype == "float64")
    e = HipEngine(6, dtype)
    try:
        e.set_wish_from_coords(xs)
        e.set_weight_power(1)
        deg, sums = e.degrees(), e.weight_sums()
    finally:
        e.close()
    print("value rule %s coords: degrees %s" % (dtype, deg.tolist()))
    _same(deg, im.degrees_of(w), (dtype, "coords", "degrees"))
    assert numpy.isfinite(sums).all()
    assert (numpy.abs(sums - im.weight_sums_of(w, 1)) <= im.weight_sum_bound(w, 1, 0.0)).all()
