"""GPU: the 24-bit stream of the fp32 stress sweep (docs/SPEC.md 3.7) where tests/test_gpu_pack24.py
does not take it: tile lists, strip changes inside a wave's chunk, several maps in one solver,
ranks of a tile list, a second map written into an engine that has built a stream, and the calls
that stand next to the sweep.  By default the stream exists only above 240 MB of units per rank;
here BB_PACK24=1 builds it on maps of at most 5,120 bins.

Every case runs twice, BB_PACK24=1 and BB_PACK24=0, and the two runs are held to EQUAL BITS:
coordinates, every stress history entry, the exchange buffer of one grad() and stress().  Every
case also shows that what it is about happened on this device: `stream_info()` equals the numpy
model (tests/_pack24_model.py), units were packed, and where a case is about a strip change
inside a chunk, the chunk rule evaluated for this device's CU count says that some wave has one
of the wanted kind.  No case skips: a device on which a precondition cannot be met fails it.

Where a float64 reference is involved (tests/_pack24_model.stress_grad / run over the stored
cells), the tolerance is SPEC 4's fp32 1e-5: on the gradient relative to its largest entry, on
the stress, and on histories and coordinates."""
import ctypes

import numpy
import pytest

import blueberry_amd as bb
from blueberry_amd import _lib
from blueberry_amd.solver import DeviceTriples, GroupEngine, HipEngine, tiles_from_entries
from tests import _many_model as mm
from tests import _oracle
from tests import _pack24_model as pm
from tests._pack24_model import RPU, UPT, VW
from tests._pack24_model import uniform_map as _uniform_map
from tests._ranks import no_rank_process_outlives_its_test as _no_rank_process_outlives_its_test    # noqa: F401
from tests._util import cu_count as _cu_count
from tests.test_gpu_pack24 import _env, _same

pytestmark = pytest.mark.gpu

TOL = 1e-5                                            # SPEC 4, fp32


# ---- what a run leaves, and how two runs compare ------------------------------------------------------
def _measure(eng, x0, lr, k=5, mus=(0.0,), loop=False, stress=True):
    """One gradient's exchange buffer (one map), stress() and stress_maps(), and for every momentum
    the coordinates and the history after k steps (iterate, or grad + apply when `loop`)."""
    out = {}
    if eng.n_maps == 1:                                # (a solver of several maps refuses grad())
        eng.set_coords(x0)
        eng.grad()
        eng.sync()
        out["grad"] = eng.read_exchange()
    eng.set_coords(x0)                                 # (drops the pending gradient)
    if stress:
        out["stress"] = numpy.array([eng.stress()])
        out["stress_maps"] = eng.stress_maps()
    for mu in mus:
        eng.set_coords(x0)
        eng.set_momentum(mu)
        if loop:
            for _ in range(k):
                eng.grad()
                eng.apply(lr)
        else:
            eng.iterate(k, lr)
            assert eng.iteration_path() == ("units", 0)
        out["X", mu] = eng.get_coords()
        out["hist", mu] = eng.stress_history()
        assert out["hist", mu].shape == (k * eng.n_maps,)
    return out


def _assert_same_bits(a, b, what):
    assert sorted(map(str, a)) == sorted(map(str, b)), what
    for key in a:
        assert _same(a[key], b[key]), (what, key)


def _twins(monkeypatch, env, scenario):
    """scenario() with the stream and without it; returns (on, off)."""
    _env(monkeypatch, BB_PACK24=1, **env)
    on = scenario(True)
    _env(monkeypatch, BB_PACK24=0, **env)
    off = scenario(False)
    return on, off


def _no_stream(n_local):
    return {"packed_units": 0, "raw_units": n_local, "stream_bytes": 0, "format_switches": 0}


def _check_info(eng, want, on):
    """stream_info() and the bytes traffic() says a sweep reads: the model's with the stream, the
    raw units' without."""
    lay = eng.layout()
    n_local = lay["u_end"] - lay["u_begin"]
    info = eng.stream_info()
    if on:
        assert info == want, (info, want)
        assert eng.traffic()["unit_bytes"] == (want["stream_bytes"] or n_local * 8192)
    else:
        assert info == _no_stream(n_local)
        assert eng.traffic()["unit_bytes"] == n_local * 8192
    return info


def _report(what, info, **errors):
    print("%s: %d packed / %d raw units, %d format switches%s"
          % (what, info["packed_units"], info["raw_units"], info["format_switches"],
             "".join("; %s %.2e" % (k, v) for k, v in sorted(errors.items()))))


def _cell(tiles, u, row=1, col=37):
    """A cell (i, j) of unit u of a tile list."""
    t, sub = divmod(u, UPT)
    return int(tiles[0][t]) * VW + sub * RPU + row, int(tiles[1][t]) * VW + col


def _plant(w, tiles, units, off=0):
    """A 0 in one cell of each of `units` (both triangles); w's bin 0 is the solver's bin off."""
    for u in units:
        i, j = _cell(tiles, u)
        w[i - off, j - off] = w[j - off, i - off] = 0.0


def _grad_error(ex, g_ref, S_ref, n):
    got = ex[:3 * n].reshape(n, 3)
    return (float(numpy.abs(got - g_ref).max() / numpy.abs(g_ref).max()),
            float(abs(ex[-2] + ex[-1] - S_ref) / S_ref))


# ---- a. a tile list without diagonal tiles, one map ------------------------------------------------------
NA = 10 * VW
TILES_A = (numpy.arange(0, 10, 2, dtype=numpy.int32), numpy.arange(1, 10, 2, dtype=numpy.int32))
UNITS_A = 5 * UPT
LR_A = 1.0 / (2.0 * 2 * VW)


def _blocks_a(seed=0):
    """Five blocks of 1,024 bins; with TILES_A only each block's tile (0, 1) is stored."""
    return [_uniform_map(2 * VW, seed=seed + m) for m in range(5)]


def _whole(blocks, n=NA):
    """The whole matrix of blocks laid end to end (only the blocks' pages are ever touched)."""
    w = numpy.zeros((n, n))
    for m, b in enumerate(blocks):
        w[m * 2 * VW:m * 2 * VW + b.shape[0], m * 2 * VW:m * 2 * VW + b.shape[0]] = b
    return w


def _write_blocks(eng, blocks):
    for m, b in enumerate(blocks):
        eng.set_wish_dense_block(b, m * 2 * VW, "wish", 1.0)


@pytest.fixture(scope="module")
def start_a():
    return _oracle.noisy_init(_oracle.random_walk(NA))


def _inside_changes(n_local, strips, wpc):
    """(chunks, the units u at which a strip changes INSIDE a wave's chunk) on this device."""
    cus = _cu_count()
    ch = pm.chunks(n_local, cus, wpc, pm.waves_per_block(n_local, cus, wpc))
    inside = [u for a, b in ch for u in range(a + 1, b) if strips[u] != strips[u - 1]]
    return ch, inside, cus


PLANTS_A = ["none", "format_change", "raw_pair"]


@pytest.mark.parametrize("plant", PLANTS_A)
def test_tile_list_strip_changes_inside_a_chunk(monkeypatch, start_a, plant):
    """640 packable units in five strips, one wave per CU: chunks of 2 to 3 units, some of which
    straddle a multiple of 128.  'none': a strip change inside a packed run.  'format_change': a raw
    unit immediately before one such change and immediately behind another.  'raw_pair': raw units
    on both sides of one.  Against the float64 reference: gradient, stress, 7 steps at momentum 0
    and 0.5."""
    strips = pm.strip_of_unit(NA, TILES_A)
    ch, inside, cus = _inside_changes(UNITS_A, strips, 1)
    assert len(inside) >= 2, ("with %d CUs no two strip changes of the five-strip tile list lie inside a "
                              "wave's chunk (%r): this case cannot be made on this device" % (cus, inside))
    blocks = _blocks_a()
    raw = {"none": [], "format_change": [inside[0] - 1, inside[1]],
           "raw_pair": [inside[0] - 1, inside[0]]}[plant]
    for u in raw:
        m = u // UPT
        _plant(blocks[m], TILES_A, [u], off=m * 2 * VW)
    min_run = 64 if plant == "none" else 1           # 'none': the default run rule
    w = _whole(blocks)
    want, packed, _ = pm.model(w, NA, 0, UNITS_A, min_run, TILES_A)
    assert not packed[raw].any() and want["packed_units"] == UNITS_A - len(raw)
    cross = pm.crossings(ch, strips, packed)
    if plant == "none":
        assert cross["packed"], "no wave holds a strip change inside a packed run (%d CUs)" % cus
    elif plant == "format_change":
        assert cross["raw_packed"] and cross["packed_raw"], (cross, cus)
    else:
        assert cross["raw"], (cross, cus)

    def scenario(on):
        eng = HipEngine(NA, "float32", tiles=TILES_A)
        try:
            _write_blocks(eng, blocks)
            info = _check_info(eng, want, on)
            assert eng.layout()["n_units"] == UNITS_A
            return info, _measure(eng, start_a, LR_A, k=7, mus=(0.0, 0.5))
        finally:
            eng.close()

    env = {"BB_WAVES_PER_CU": 1}
    if plant != "none":
        env["BB_PACK24_MIN_RUN"] = min_run
    (info, on), (_, off) = _twins(monkeypatch, env, scenario)
    assert info["packed_units"] > 0
    _assert_same_bits(on, off, plant)
    S_ref, g_ref = pm.stress_grad(w, NA, start_a, TILES_A)
    err_g, err_s = _grad_error(on["grad"], g_ref, S_ref, NA)
    err_s = max(err_s, abs(on["stress"][0] / S_ref - 1))
    worst_h = worst_x = 0.0
    for mu in (0.0, 0.5):
        X_ref, h_ref = pm.run(w, NA, start_a, 7, LR_A, mu=mu, tiles=TILES_A)
        worst_h = max(worst_h, float(numpy.abs(on["hist", mu] / h_ref - 1).max()))
        worst_x = max(worst_x, float(numpy.abs(on["X", mu] - X_ref).max() / numpy.abs(X_ref).max()))
    _report("tile list, %s, crossings %r" % (plant, {k: len(v) for k, v in cross.items()}), info,
            gradient=err_g, stress=err_s, history=worst_h, coordinates=worst_x)
    assert err_g < TOL and err_s < TOL and worst_h < TOL and worst_x < TOL


@pytest.mark.parametrize("wpc", [4, 8])
def test_tile_list_both_workgroup_forms(monkeypatch, start_a, wpc):
    """The tile list under workgroups of 4 waves and of 8 (paired): the first descriptor of every
    wave comes from the table, the row partials start at the rank's first tile."""
    blocks = _blocks_a()
    _plant(blocks[1], TILES_A, [UPT + 9, UPT + 10, 2 * UPT - 1], off=2 * VW)
    w = _whole(blocks)
    want, _, _ = pm.model(w, NA, 0, UNITS_A, 1, TILES_A)
    cus = _cu_count()
    assert pm.waves_per_block(UNITS_A, cus, wpc) == wpc

    def scenario(on):
        eng = HipEngine(NA, "float32", tiles=TILES_A)
        try:
            _write_blocks(eng, blocks)
            return _check_info(eng, want, on), _measure(eng, start_a, LR_A, k=7, mus=(0.0, 0.5))
        finally:
            eng.close()

    (info, on), (_, off) = _twins(monkeypatch, {"BB_PACK24_MIN_RUN": 1, "BB_WAVES_PER_CU": wpc}, scenario)
    assert info["packed_units"] == UNITS_A - 3
    _assert_same_bits(on, off, wpc)
    S_ref, g_ref = pm.stress_grad(w, NA, start_a, TILES_A)
    err_g, err_s = _grad_error(on["grad"], g_ref, S_ref, NA)
    X_ref, h_ref = pm.run(w, NA, start_a, 7, LR_A, mu=0.5, tiles=TILES_A)
    err_h = float(numpy.abs(on["hist", 0.5] / h_ref - 1).max())
    err_x = float(numpy.abs(on["X", 0.5] - X_ref).max() / numpy.abs(X_ref).max())
    _report("tile list, %d waves per CU" % wpc, info, gradient=err_g, stress=err_s, history=err_h,
            coordinates=err_x)
    assert err_g < TOL and err_s < TOL and err_h < TOL and err_x < TOL


# ---- b. the same tile list as five maps ---------------------------------------------------------------------
BEGIN_B = [m * 2 * VW for m in range(6)]
FREE_B = 8                                  # the first bins of every map carry no pair and never move


def _maps_b(seed=10):
    """Map m: a uniform map of 1,024 bins at 2^(m mod 7) times the scale of map 0, its first 8 bins
    without a pair (units 0 and 1 of its tile are all zero: packed with base 0), and its start."""
    maps, starts = [], []
    for m in range(5):
        w = _uniform_map(2 * VW, seed=seed + m) * mm.map_scale(m)
        w[:FREE_B, :] = 0.0
        w[:, :FREE_B] = 0.0
        x = _oracle.noisy_init(_oracle.random_walk(2 * VW, seed=seed + m), seed=seed + 50 + m) * mm.map_scale(m)
        x[:FREE_B] = 0.0
        maps.append(w)
        starts.append(x)
    return maps, starts


def _run_maps(on, maps, starts, want, lr_scale, bin_steps, mu, k, other=None):
    """The five maps in one engine: stress_maps before the first step, k steps; then (other =
    (m, map, its model)) map m written again and k more steps from the same start."""
    eng = HipEngine(NA, "float32", tiles=TILES_A)
    try:
        eng.set_maps(BEGIN_B, lr_scale)
        _write_blocks(eng, maps)
        if bin_steps is not None:
            eng.set_bin_steps(bin_steps)
        info = _check_info(eng, want, on)
        x0 = numpy.concatenate(starts)
        out = _measure(eng, x0, LR_A, k=k, mus=(mu,))
        if other is not None:
            m, w_other, want_other = other
            eng.set_wish_dense_block(w_other, BEGIN_B[m], "wish", 1.0)
            _check_info(eng, want_other, on)
            for key, v in _measure(eng, x0, LR_A, k=k, mus=(mu,)).items():
                out[("other",) + (key if isinstance(key, tuple) else (key,))] = v
        return info, out
    finally:
        eng.close()


@pytest.mark.parametrize("steps", ["per_map", "per_bin"])
def test_five_maps_on_the_tile_list(monkeypatch, steps):
    """Every map's stress and history against the reference of that map ALONE, and bit for bit
    against the run without the stream; one wave per CU, so that waves leave a map behind
    mid-chunk and its stress partial goes out through the stream loop's own strip store."""
    k = 4
    maps, starts = _maps_b()
    w = _whole(maps)
    want, packed, _ = pm.model(w, NA, 0, UNITS_A, 1, TILES_A)
    assert want["packed_units"] == UNITS_A and want["raw_units"] == 0
    strips = pm.strip_of_unit(NA, TILES_A)
    ch, inside, cus = _inside_changes(UNITS_A, strips, 1)
    assert pm.crossings(ch, strips, packed)["packed"], \
        "no wave holds units of two maps inside a packed run (%d CUs)" % cus
    if steps == "per_map":
        lr_scale, bin_steps, mu = [1.0, 0.9, 0.8, 0.7, 0.6], None, 0.0
    else:
        lr_scale, mu = [1.0] * 5, 0.3
        bin_steps = numpy.random.default_rng(3).uniform(0.5, 1.0, NA).astype(numpy.float32).astype(numpy.float64)
    odd = 2
    w_other = _uniform_map(2 * VW, seed=77) * mm.map_scale(odd)
    w_other[:FREE_B, :] = 0.0
    w_other[:, :FREE_B] = 0.0
    _plant(w_other, TILES_A, [odd * UPT + 40], off=BEGIN_B[odd])
    want_other = pm.model(_whole(maps[:odd] + [w_other] + maps[odd + 1:]), NA, 0, UNITS_A, 1, TILES_A)[0]
    assert want_other["raw_units"] == 1

    (info, on), (_, off) = _twins(
        monkeypatch, {"BB_PACK24_MIN_RUN": 1, "BB_WAVES_PER_CU": 1},
        lambda flag: _run_maps(flag, maps, starts, want, lr_scale, bin_steps, mu, k, (odd, w_other, want_other)))
    assert info["packed_units"] > 0
    _assert_same_bits(on, off, steps)
    hist = on["hist", mu].reshape(k, 5)
    X = on["X", mu]
    worst = {"stress_maps": 0.0, "history": 0.0, "coordinates": 0.0}
    tile01 = (numpy.array([0]), numpy.array([1]))
    for m in range(5):
        lo, hi = BEGIN_B[m], BEGIN_B[m + 1]
        scale = None if bin_steps is None else bin_steps[lo:hi]
        X_ref, h_ref = pm.run(maps[m], 2 * VW, starts[m], k, LR_A * lr_scale[m], mu=mu, bin_scale=scale,
                              tiles=tile01)
        S_ref = pm.stress_grad(maps[m], 2 * VW, starts[m], tile01)[0]
        assert S_ref == h_ref[0]
        worst["stress_maps"] = max(worst["stress_maps"], abs(on["stress_maps"][m] / S_ref - 1))
        worst["history"] = max(worst["history"], float(numpy.abs(hist[:, m] / h_ref - 1).max()))
        worst["coordinates"] = max(worst["coordinates"],
                                   float(numpy.abs(X[lo:hi] - X_ref).max() / numpy.abs(X_ref).max()))
        # the rows without a pair never move: exactly 0
        assert not X[lo:lo + FREE_B].any()
    _report("five maps, steps %s" % steps, info, **worst)
    assert max(worst.values()) < TOL, worst
    assert abs(on["stress"][0] / on["stress_maps"].sum() - 1) < 1e-12
    # map 2 written again: every other map's numbers are the bits they were
    hist2 = on["other", "hist", mu].reshape(k, 5)
    X2 = on["other", "X", mu]
    for m in range(5):
        lo, hi = BEGIN_B[m], BEGIN_B[m + 1]
        same = _same(hist2[:, m], hist[:, m]) and _same(X2[lo:hi], X[lo:hi]) and \
            _same(on["other", "stress_maps"][m], on["stress_maps"][m])
        assert same == (m != odd), m
    scale = None if bin_steps is None else bin_steps[BEGIN_B[odd]:BEGIN_B[odd + 1]]
    X_ref, h_ref = pm.run(w_other, 2 * VW, starts[odd], k, LR_A * lr_scale[odd], mu=mu, bin_scale=scale,
                          tiles=tile01)
    assert numpy.abs(hist2[:, odd] / h_ref - 1).max() < TOL
    assert numpy.abs(X2[BEGIN_B[odd]:BEGIN_B[odd + 1]] - X_ref).max() < TOL * numpy.abs(X_ref).max()


def test_fit_many_with_the_stream(monkeypatch):
    """StructureSolver.fit_many(kind='wish') on maps of 1,024 and 1,536 bins of uniform distances,
    laid out by `_many_model.joint_layout` (diagonal tiles present): stream on against stream off."""
    sizes, k = (2 * VW, 3 * VW), 4
    lay = mm.joint_layout(sizes, "float32")
    maps = [_uniform_map(n, seed=20 + m) * mm.map_scale(m + 1) for m, n in enumerate(sizes)]
    # compact starts: from a start far outside the wish distances the first full Guttman step
    # (lr = 1 / 2N on a complete map) cancels two digits of the fp32 coordinates
    starts = [0.8 * numpy.random.default_rng(60 + m).standard_normal((n, 3)) * mm.map_scale(m + 1)
              for m, n in enumerate(sizes)]
    w = numpy.zeros((lay["total"], lay["total"]))
    for o, m in zip(lay["off"], maps):
        w[o:o + m.shape[0], o:o + m.shape[0]] = m
    want, _, _ = pm.model(w, lay["total"], 0, lay["n_units"], 64, lay["tiles"])
    assert want["packed_units"] == 4 * UPT and want["raw_units"] == 5 * UPT

    def scenario(on):
        # the layout fit_many gives the batch, in an engine of our own: what the stream holds there
        eng = HipEngine(lay["total"], "float32", tiles=lay["tiles"])
        try:
            eng.set_maps(lay["off"] + [lay["total"]], [1.0, 1.0])
            for o, m in zip(lay["off"], maps):
                eng.set_wish_dense_block(m, o, "wish", 1.0)
            info = _check_info(eng, want, on)
        finally:
            eng.close()
        s = bb.StructureSolver(n_iter=k, dtype="float32", kind="wish").fit_many(maps, inits=starts)
        out = {}
        for m in range(2):
            out["X", m], out["hist", m] = s.structures_[m], s.stresses_[m]
            assert s.stresses_[m].shape == (k,)
        return info, out

    (info, on), (_, off) = _twins(monkeypatch, {}, scenario)
    assert info["packed_units"] > 0
    _assert_same_bits(on, off, "fit_many")
    worst = 0.0
    for m, n in enumerate(sizes):
        X_ref, h_ref = pm.run(maps[m], n, starts[m], k, 1.0 / (2.0 * n))
        worst = max(worst, float(numpy.abs(on["hist", m] / h_ref - 1).max()),
                    float(numpy.abs(on["X", m] - X_ref).max() / numpy.abs(X_ref).max()))
    _report("fit_many of 1,024 and 1,536 bins", info, worst=worst)
    assert worst < TOL


# ---- c. tile lists with ranks ----------------------------------------------------------------------------------
NC = 5 * VW
BAND_C = (numpy.array([0, 0, 1, 1, 2, 2, 3, 1, 2, 3, 4], dtype=numpy.int32),
          numpy.array([0, 1, 1, 2, 2, 3, 3, 4, 4, 4, 4], dtype=numpy.int32))


@pytest.fixture(scope="module")
def band_c():
    return _uniform_map(NC, seed=30), _oracle.noisy_init(_oracle.random_walk(NC))


@pytest.mark.parametrize("rank,world", [(1, 2), (2, 3)])
@pytest.mark.parametrize("layout", ["no_diagonal", "band"])
def test_tile_list_on_a_later_rank(monkeypatch, start_a, band_c, layout, rank, world):
    """Rank 1 of 2 and rank 2 of 3 of a tile list, grad / apply without a connect: the rank's first
    unit lies inside a tile and is packed, `rowpart` starts at the rank's first tile.  The ranks'
    exchange buffers summed are the one-rank gradient."""
    if layout == "no_diagonal":
        n, tiles, x0, lr = NA, TILES_A, start_a, LR_A
        blocks = _blocks_a()
        w = _whole(blocks)
        write = lambda e: _write_blocks(e, blocks)
    else:
        n, tiles, lr = NC, BAND_C, 1.0 / (2.0 * NC)
        w, x0 = band_c
        write = lambda e: e.set_wish_dense(w, "wish", 1.0)
    n_units = len(tiles[0]) * UPT
    a, b = pm.rank_range(n_units, rank, world)
    want, packed, _ = pm.model(w, n, a, b, 1, tiles)
    assert a % UPT != 0 and packed[0], "the rank's first unit: inside a tile, and packed"

    def run_rank(r, wld, on, steps):
        eng = HipEngine(n, "float32", rank=r, world=wld, tiles=tiles)
        try:
            write(eng)
            lay = eng.layout()
            assert (lay["u_begin"], lay["u_end"]) == pm.rank_range(n_units, r, wld)
            info = _check_info(eng, pm.model(w, n, lay["u_begin"], lay["u_end"], 1, tiles)[0], on)
            out = _measure(eng, x0, lr, k=steps, mus=(0.0, 0.5), loop=True, stress=False)
            return info, out
        finally:
            eng.close()

    env = {"BB_PACK24_MIN_RUN": 1, "BB_WAVES_PER_CU": 1}
    (info, on), (_, off) = _twins(monkeypatch, env, lambda flag: run_rank(rank, world, flag, 4))
    assert info == want and info["packed_units"] > 0
    _assert_same_bits(on, off, (layout, rank, world))
    # the ranks' buffers summed against one rank's, with the stream
    _env(monkeypatch, BB_PACK24=1, **env)
    total = sum(run_rank(r, world, True, 0)[1]["grad"] for r in range(world) if r != rank) + on["grad"]
    one = run_rank(0, 1, True, 0)[1]["grad"]
    err = float(numpy.abs(total[:-2] - one[:-2]).max() / numpy.abs(one[:-2]).max())
    err_s = abs((total[-2] + total[-1]) / (one[-2] + one[-1]) - 1)
    S_ref, g_ref = pm.stress_grad(w, n, x0, tiles, a, b)
    err_g, err_r = _grad_error(on["grad"], g_ref, S_ref, n)
    _report("%s rank %d of %d" % (layout, rank, world), info, ranks_summed=err, ranks_stress=err_s,
            gradient=err_g, stress=err_r)
    assert err < TOL and err_s < TOL and err_g < TOL and err_r < TOL


# ---- d. a second map written into an engine that has built a stream ---------------------------------------------
ND = 4 * VW
LR_D = 1.0 / (2.0 * ND)
DENSE_D = pm.dense_tiles(ND)
TWO_MAPS_D = mm.joint_layout((2 * VW, 2 * VW), "float32")["tiles"]       # (0,0) (0,1) (1,1) (2,2) (2,3) (3,3)


def _tile_index(tiles, I, J):
    return [t for t in range(len(tiles[0])) if (tiles[0][t], tiles[1][t]) == (I, J)][0]


def _maps_d(tiles, kind):
    """Maps A and B of 2,048 bins.  A has a 0 planted in two units of tile (2, 3).  B 'values': A's
    pattern with other values; B 'pattern': zeros planted where A packed, A's zeros filled."""
    t23 = _tile_index(tiles, 2, 3) * UPT
    zeros_a = [t23 + 5, t23 + 70]
    zeros_b = zeros_a if kind == "values" else [t23 + 20, t23 + 21, t23 + 100]
    wa, wb = _uniform_map(ND, seed=40), _uniform_map(ND, seed=41, hi=1.5)
    _plant(wa, tiles, zeros_a)
    _plant(wb, tiles, zeros_b)
    return wa, wb


def _triu_entries(w):
    i, j = numpy.nonzero(numpy.triu(w, 1))
    return i, j, w[i, j]


class _Writer(object):
    """One input route: first(eng, w) writes a whole map into a new engine, again(eng, w) writes
    map w into an engine that holds another one.  `composite`: what the engine then holds."""
    tiles, maps = None, None

    def engine(self):
        eng = HipEngine(ND, "float32", tiles=self.tiles)
        if self.maps is not None:
            eng.set_maps(*self.maps)
        return eng

    def layout_tiles(self):
        return DENSE_D if self.tiles is None else self.tiles

    def first(self, eng, w):
        raise NotImplementedError

    def again(self, eng, w):
        self.first(eng, w)

    def composite(self, wa, wb):
        return wb


class _Dense(_Writer):
    def first(self, eng, w):
        eng.set_wish_dense(w, "wish", 1.0)


class _DenseBlock(_Writer):
    """A block of a one-map solver: bins 1,024 .. 2,047 written again, the rest stays A."""
    def first(self, eng, w):
        eng.set_wish_dense_block(w, 0, "wish", 1.0)

    def again(self, eng, w):
        eng.set_wish_dense_block(w[2 * VW:, 2 * VW:], 2 * VW, "wish", 1.0)

    def composite(self, wa, wb):
        c = wa.copy()
        c[2 * VW:, 2 * VW:] = wb[2 * VW:, 2 * VW:]
        return c


class _DenseBlockOfMaps(_DenseBlock):
    """One map of two."""
    tiles, maps = TWO_MAPS_D, ([0, 2 * VW, ND], [1.0, 0.75])

    def first(self, eng, w):
        eng.set_wish_dense_block(w[:2 * VW, :2 * VW], 0, "wish", 1.0)
        eng.set_wish_dense_block(w[2 * VW:, 2 * VW:], 2 * VW, "wish", 1.0)

    def composite(self, wa, wb):
        c = numpy.zeros_like(wa)
        c[:2 * VW, :2 * VW] = wa[:2 * VW, :2 * VW]
        c[2 * VW:, 2 * VW:] = wb[2 * VW:, 2 * VW:]
        return c


class _Resident(_Writer):
    """set_wish_resident, which is set_wish_from_cm of the map's device copy."""
    def first(self, eng, w):
        cm = bb.ContactMap.from_matrix(w)
        dev = cm._resident()
        try:
            eng.set_wish_resident(cm, "wish", 1.0)
        finally:
            dev.close()


class _CmBlock(_DenseBlock):
    def _put(self, eng, w, off):
        dev = bb.ContactMap.from_matrix(w)._resident()
        try:
            eng.set_wish_from_cm_block(dev, off, "wish", 1.0)
        finally:
            dev.close()

    def first(self, eng, w):
        self._put(eng, w, 0)

    def again(self, eng, w):
        self._put(eng, numpy.ascontiguousarray(w[2 * VW:, 2 * VW:]), 2 * VW)


class _Sparse(_Writer):
    def first(self, eng, w):
        i, j, v = _triu_entries(w)
        eng.set_wish_sparse(i, j, v, "wish", 1.0)


class _Triples(_Writer):
    def first(self, eng, w):
        i, j, v = _triu_entries(w)
        dev = DeviceTriples(numpy.column_stack([i * 1000.0, j * 1000.0, v]), 1000, 0)
        try:
            eng.set_wish_triples(dev, "wish", 1.0)
        finally:
            dev.close()


WRITERS = {"dense": _Dense, "dense_block": _DenseBlock, "dense_block_of_maps": _DenseBlockOfMaps,
           "resident": _Resident, "cm_block": _CmBlock, "sparse": _Sparse, "triples": _Triples}
REWRITES = ([(name, kind, builder) for name in sorted(WRITERS)
             for kind, builder in (("values", "grad"), ("pattern", "stream_info"))]
            + [("dense", "values", "stream_info"), ("dense", "pattern", "grad")])


def _build_stream(eng, x0, builder):
    """By the first sweep ('grad': one grad(), or one iteration where the solver holds several maps
    and refuses grad()) or by stream_info()."""
    if builder == "grad":
        eng.set_coords(x0)
        if eng.n_maps > 1:
            eng.iterate(1, LR_D)
        else:
            eng.grad()
        eng.sync()
    else:
        eng.stream_info()


@pytest.fixture(scope="module")
def start_d():
    """A compact start: pair distances of the order of the wish distances, so that two maps'
    stresses differ by far more than the tolerance."""
    return 0.8 * numpy.random.default_rng(11).standard_normal((ND, 3))


def _rewrite_scenario(on, wr, write_a, write_b, write_b_fresh, want_a, want_b, x0, builder):
    """An engine that built a stream of A and was then given B, and one that only ever saw B."""
    eng = wr.engine()
    try:
        write_a(eng)
        _build_stream(eng, x0, builder)
        if want_a is not None:
            _check_info(eng, want_a, on)
        elif on:
            assert eng.stream_info()["packed_units"] > 0
        write_b(eng)
        out = _measure(eng, x0, LR_D)
        info = eng.stream_info() if want_b is None else _check_info(eng, want_b, on)
    finally:
        eng.close()
    eng = wr.engine()
    try:
        write_b_fresh(eng)
        fresh = _measure(eng, x0, LR_D)
        assert eng.stream_info() == info and (want_b is None or _check_info(eng, want_b, on))
    finally:
        eng.close()
    _assert_same_bits(out, fresh, "after the rewrite against a fresh engine")
    return info, out


@pytest.mark.parametrize("name,kind,builder", REWRITES)
def test_rewrite_through_every_writer(monkeypatch, start_d, name, kind, builder):
    """Map A, the stream built (by one grad() or by stream_info(), itself a builder), then map B
    through the same writer: gradient, stress() and 5 steps are the bits of an engine that only
    ever saw B and of the twin without the stream; stream_info() and traffic() are B's."""
    wr = WRITERS[name]()
    tiles = wr.layout_tiles()
    wa, wb = _maps_d(tiles, kind)
    comp = wr.composite(wa, wb)
    if wr.maps is not None:
        wa = wr.composite(wa, wa)
    n_units = len(tiles[0]) * UPT
    want_a = pm.model(wa, ND, 0, n_units, 1, tiles)[0]
    want_b = pm.model(comp, ND, 0, n_units, 1, tiles)[0]
    assert want_a["raw_units"] == want_b["raw_units"] - (kind == "pattern")
    (info, on), (_, off) = _twins(
        monkeypatch, {"BB_PACK24_MIN_RUN": 1},
        lambda flag: _rewrite_scenario(flag, wr, lambda e: wr.first(e, wa), lambda e: wr.again(e, wb),
                                       lambda e: wr.first(e, comp), want_a, want_b, start_d, builder))
    assert info == want_b and info["packed_units"] > 0
    _assert_same_bits(on, off, (name, kind, builder))
    # and B is not A: the sweep of the old stream would have given other bits
    S_a = pm.stress_grad(wa, ND, start_d, tiles)[0]
    S_b, g_b = pm.stress_grad(comp, ND, start_d, tiles)
    assert abs(S_a / S_b - 1) > 100 * TOL
    err_g, err_s = _grad_error(on["grad"], g_b, S_b, ND) if "grad" in on else (0.0, 0.0)
    err_s = max(err_s, abs(on["stress"][0] / S_b - 1))
    _report("rewrite %s, B %s, built by %s" % (name, kind, builder), info, gradient=err_g, stress=err_s)
    assert err_g < TOL and err_s < TOL


@pytest.mark.parametrize("kind,builder", [("values", "grad"), ("pattern", "stream_info")])
def test_rewrite_from_coordinates(monkeypatch, start_d, kind, builder):
    """set_wish_from_coords twice.  The device forms these distances itself, so `stream_info` is
    held against the fresh engine's and the twin, not against the model.  'pattern': bins made to
    coincide in B (no constraint: zeros where A packed) and A's coincident bins moved apart."""
    xa = _oracle.random_walk(ND, seed=5)
    xb = _oracle.random_walk(ND, seed=6) if kind == "values" else xa * 1.25
    xa[700] = xa[1900]                                  # a 0 in unit (700 / 4) of tile (1, 3)
    if kind == "values":
        xb[700] = xb[1900]
    else:
        xb[300] = xb[1300]
        xb[301] = xb[1301]
    wr = _Dense()
    (info, on), (_, off) = _twins(
        monkeypatch, {"BB_PACK24_MIN_RUN": 1},
        lambda flag: _rewrite_scenario(flag, wr, lambda e: e.set_wish_from_coords(xa),
                                       lambda e: e.set_wish_from_coords(xb),
                                       lambda e: e.set_wish_from_coords(xb), None, None, start_d, builder))
    assert info["packed_units"] > 0 and info["raw_units"] > 4 * UPT
    _assert_same_bits(on, off, (kind, builder))
    wb = _oracle.wish_from_coords(xb).astype(numpy.float32).astype(numpy.float64)
    S_b, g_b = pm.stress_grad(wb, ND, start_d)
    S_a = pm.stress_grad(_oracle.wish_from_coords(xa).astype(numpy.float32).astype(numpy.float64), ND, start_d)[0]
    assert abs(S_a / S_b - 1) > 100 * TOL
    err_g, err_s = _grad_error(on["grad"], g_b, S_b, ND)
    _report("rewrite from coordinates, B %s, built by %s" % (kind, builder), info, gradient=err_g, stress=err_s)
    assert err_g < TOL and err_s < TOL


def test_set_maps_on_an_engine_with_a_stream(monkeypatch, start_d):
    """bb_solver_set_maps clears the units and never reaches the writers' common end: before any
    map is written the stress and the gradient are exactly 0, and the stream is that of all-zero
    units (every unit packed with base 0)."""
    wa = _DenseBlockOfMaps().composite(*[_uniform_map(ND, seed=40)] * 2)
    n_units = len(TWO_MAPS_D[0]) * UPT
    want_a = pm.model(wa, ND, 0, n_units, 1, TWO_MAPS_D)[0]
    want_0 = pm.model(numpy.zeros((ND, ND)), ND, 0, n_units, 1, TWO_MAPS_D)[0]
    assert want_0 == {"packed_units": n_units, "raw_units": 0, "stream_bytes": n_units * 6144, "format_switches": 0}
    _env(monkeypatch, BB_PACK24=1, BB_PACK24_MIN_RUN=1)
    eng = HipEngine(ND, "float32", tiles=TWO_MAPS_D)
    try:
        eng.set_wish_dense_block(wa[:2 * VW, :2 * VW], 0, "wish", 1.0)
        eng.set_wish_dense_block(wa[2 * VW:, 2 * VW:], 2 * VW, "wish", 1.0)
        _build_stream(eng, start_d, "grad")
        info = _check_info(eng, want_a, True)
        assert info["packed_units"] > 0
        eng.set_coords(start_d)
        assert eng.stress() > 0.0
        eng.set_maps([0, 2 * VW, ND], [1.0, 1.0])
        eng.set_coords(start_d)
        before = eng.get_coords()
        assert eng.stress() == 0.0 and not eng.stress_maps().any()
        _check_info(eng, want_0, True)
        # (several maps: no grad(); a gradient that is exactly 0 leaves every coordinate where it was)
        eng.iterate(2, LR_D)
        assert _same(eng.get_coords(), before) and numpy.abs(before).max() > 1.0
        assert eng.stress_history().shape == (4,) and not eng.stress_history().any()
        _report("set_maps on an engine with a stream", eng.stream_info())
    finally:
        eng.close()


def _attempt(log, name, fn):
    """Run fn(); what it returned or raised goes to the log."""
    try:
        log.append((name, "ok", fn()))
    except Exception as exc:                            # noqa: BLE001 -- compared between the twins
        log.append((name, "raised", type(exc).__name__ + ": " + str(exc)))


def test_a_writer_that_fails_after_clearing_the_units(monkeypatch, start_d):
    """set_wish_sparse with an index >= n raises after the units were cleared.  What the engine does
    next is not defined here; it is the same, call for call, with and without the stream."""
    wa = _uniform_map(ND, seed=40)

    def scenario(on):
        log = []
        eng = HipEngine(ND, "float32")
        try:
            eng.set_wish_dense(wa, "wish", 1.0)
            _build_stream(eng, start_d, "grad")
            assert (eng.stream_info()["packed_units"] > 0) == on
            with pytest.raises(ValueError, match="outside"):
                eng.set_wish_sparse([0, 5], [1, ND], [1.5, 1.5], "wish", 1.0)
            _attempt(log, "set_coords", lambda: eng.set_coords(start_d))
            _attempt(log, "grad", lambda: (eng.grad(), eng.sync(), eng.read_exchange())[2])
            _attempt(log, "set_coords", lambda: eng.set_coords(start_d))
            _attempt(log, "stress", eng.stress)
            _attempt(log, "iterate", lambda: eng.iterate(3, LR_D))
            _attempt(log, "get_coords", eng.get_coords)
            _attempt(log, "history", eng.stress_history)
            _attempt(log, "units", lambda: sum(eng.stream_info()[k] for k in ("packed_units", "raw_units")))
        finally:
            eng.close()
        return log

    on, off = _twins(monkeypatch, {"BB_PACK24_MIN_RUN": 1}, scenario)
    assert [e[:2] for e in on] == [e[:2] for e in off]
    for (name, how, a), (_, _, b) in zip(on, off):
        if how == "raised" or a is None:
            assert a == b, name
        else:
            assert _same(a, b), name
    print("a failed writer, then: " + ", ".join("%s %s" % e[:2] for e in on))


# ---- e. the neighbours of the sweep ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def maps_e():
    return _maps_d(DENSE_D, "pattern")


def test_weight_power_and_back(monkeypatch, start_d, maps_e):
    """q = 0 -> 2 -> 0: the weighted sweeps read the units (equal on / off); back at q = 0 the stream
    is in use again, unchanged; a map written while q = 2 is the one the stream holds at q = 0."""
    wa, wb = maps_e
    want_a = pm.model(wa, ND, 0, 10 * UPT, 1)[0]
    want_b = pm.model(wb, ND, 0, 10 * UPT, 1)[0]

    def scenario(on):
        out = {}
        eng = HipEngine(ND, "float32")
        try:
            eng.set_wish_dense(wa, "wish", 1.0)
            info = _check_info(eng, want_a, on)
            first = _measure(eng, start_d, LR_D, k=3)
            eng.set_weight_power(2)
            for key, v in _measure(eng, start_d, LR_D, k=3).items():
                out["q2", str(key)] = v
            eng.set_weight_power(0)
            assert eng.stream_info() == info
            back = _measure(eng, start_d, LR_D, k=3)
            _assert_same_bits(back, first, "back at q = 0")
            for key, v in back.items():
                out["q0", str(key)] = v
            eng.set_weight_power(2)
            eng.set_wish_dense(wb, "wish", 1.0)
            eng.set_weight_power(0)
            after = _measure(eng, start_d, LR_D, k=3)
            _check_info(eng, want_b, on)
        finally:
            eng.close()
        eng = HipEngine(ND, "float32")
        try:
            eng.set_wish_dense(wb, "wish", 1.0)
            _assert_same_bits(after, _measure(eng, start_d, LR_D, k=3), "B written while q = 2")
        finally:
            eng.close()
        for key, v in after.items():
            out["B", str(key)] = v
        return info, out

    (info, on), (_, off) = _twins(monkeypatch, {"BB_PACK24_MIN_RUN": 1}, scenario)
    assert info["packed_units"] > 0
    _assert_same_bits(on, off, "weight power")
    assert not _same(on["q2", "grad"], on["q0", "grad"]) and not _same(on["B", "grad"], on["q0", "grad"])
    _report("weight power 0 -> 2 -> 0", info)


def test_score_matvec_and_spectral_start_beside_the_stream(monkeypatch, start_d, maps_e):
    """score(), matvec_sq and spectral_init_device read the units: equal on / off, and a sweep
    after them is the sweep before them."""
    wa = maps_e[0]
    want = pm.model(wa, ND, 0, 10 * UPT, 1)[0]
    v0 = numpy.random.default_rng(9).standard_normal((ND, 3))

    def scenario(on):
        eng = HipEngine(ND, "float32")
        try:
            eng.set_wish_dense(wa, "wish", 1.0)
            info = _check_info(eng, want, on)
            out = _measure(eng, start_d, LR_D, k=3)
            out["profile"], out["bins"] = eng.score(start_d)
            out["matvec"] = eng.matvec_sq(v0)
            done, res = eng.spectral_init_device(6, v0)
            out["spectral"] = numpy.concatenate([[done, res], eng.get_coords().ravel()])
            _assert_same_bits(_measure(eng, start_d, LR_D, k=3), {k: out[k] for k in out if k in (
                "grad", "stress", "stress_maps", ("X", 0.0), ("hist", 0.0))}, "a sweep after the neighbours")
            assert eng.stream_info() == info
            return info, out
        finally:
            eng.close()

    (info, on), (_, off) = _twins(monkeypatch, {"BB_PACK24_MIN_RUN": 1}, scenario)
    assert info["packed_units"] > 0 and numpy.count_nonzero(on["matvec"]) > 0
    _assert_same_bits(on, off, "neighbours")
    _report("score, matvec, spectral start", info)


@pytest.mark.parametrize("path", ["iterate", "grad_apply", "group_of_one"])
def test_exchange_paths_at_world_1(monkeypatch, start_d, maps_e, path):
    """iterate, the grad / apply loop and a GroupEngine of one member all launch the sweep through
    the one place that takes the stream (bb_solver_iterate_dist's loop: the next test)."""
    wa = maps_e[0]
    want = pm.model(wa, ND, 0, 10 * UPT, 1)[0]
    k = 5

    def scenario(on):
        if path == "group_of_one":
            g = GroupEngine(ND, "float32", [0])
            eng = g.members[0]
        else:
            g = eng = HipEngine(ND, "float32")
        try:
            g.set_wish_dense(wa, "wish", 1.0)
            info = _check_info(eng, want, on)
            g.set_coords(start_d)
            g.set_momentum(0.5)
            if path == "grad_apply":
                for _ in range(k):
                    eng.grad()
                    eng.apply(LR_D)
            else:
                g.iterate(k, LR_D)
            g.sync()
            hist = g.stress_history()
            assert hist.shape == (k,)
            return info, {"X": g.get_coords(), "hist": hist}
        finally:
            g.close()

    (info, on), (_, off) = _twins(monkeypatch, {"BB_PACK24_MIN_RUN": 1}, scenario)
    assert info["packed_units"] > 0
    _assert_same_bits(on, off, path)
    X_ref, h_ref = pm.run(wa, ND, start_d, k, LR_D, mu=0.5)
    err_h = float(numpy.abs(on["hist"] / h_ref - 1).max())
    err_x = float(numpy.abs(on["X"] - X_ref).max() / numpy.abs(X_ref).max())
    _report("world 1 through " + path, info, history=err_h, coordinates=err_x)
    assert err_h < TOL and err_x < TOL


def test_anchored_fit_with_the_stream(monkeypatch):
    """Landmark constraints beside the stream: a complete 'wish' map of 1,025 nodes given as triples
    (the units of tile (0, 1) pack), 8 kept landmarks.  The exchange
    buffer after grad() and 5 anchored steps: equal on / off, and against tests/_anchor_model.py
    at the tolerances of tests/test_gpu_anchors.py."""
    from tests import _anchor_model as am
    from tests import _input_model as im
    from tests import _landmark_model as lm
    n, lam, k = 2 * VW + 1, 0.5, 5
    w = _uniform_map(n, seed=50)
    i, j, v = _triu_entries(w)
    triples = numpy.column_stack([i.astype(float), j.astype(float), v])
    rng = numpy.random.default_rng(51)
    sources = rng.choice(n, 8, replace=False)
    kept = numpy.ones(8, dtype=bool)
    g = lm.geodesics(lm.weights_of(triples, 1, n, kind="wish"), sources)
    A, nodes = am.anchors_of(g, sources, kept, "float32")
    wm = im.matrix_of("triples", n, "float32", kind="wish", triples=triples, resolution=1)
    terms = am.Terms(wm, A, nodes, lam)
    lr, factors = am.steps_of(am.sums_of(terms, 0)[0])
    X0 = (0.8 * rng.standard_normal((n, 3))).astype(numpy.float32).astype(numpy.float64)
    # block 2 holds node 1,024 alone: no pair inside it, so the triples' tile list has no tile (2, 2)
    tiles = tiles_from_entries(n, i, j, "float32")
    assert list(zip(*tiles)) == [(0, 0), (0, 1), (1, 1), (0, 2), (1, 2)]
    want, packed, _ = pm.model(w, n, 0, 5 * UPT, 1, tiles)
    assert packed[UPT:2 * UPT].all() and want["packed_units"] == UPT

    def scenario(on):
        dev = DeviceTriples(triples, 1, 0)
        try:
            assert set(zip(*dev.tiles(n, "float32"))) == set(zip(*tiles))
            eng = HipEngine(n, "float32", tiles=tiles)
            try:
                eng.set_wish_triples(dev, "wish", 1.0)
                with dev.shortest_paths(n, sources, kind="wish") as rows:
                    eng.set_anchors(rows, kept, lam)
                assert eng.anchored and eng.anchor_info()[0] == 8
                info = _check_info(eng, want, on)
                eng.set_bin_steps(factors)
                out = _measure(eng, X0, lr, k=k, mus=(0.0,), stress=False)
                out["stress"] = numpy.array([eng.stress(), eng.anchor_stress()])
                return info, out
            finally:
                eng.close()
        finally:
            dev.close()

    (info, on), (_, off) = _twins(monkeypatch, {"BB_PACK24_MIN_RUN": 1}, scenario)
    assert info["packed_units"] > 0
    _assert_same_bits(on, off, "anchors")
    S, _, grad = am.objective(X0, terms, 0, "float32")
    f = factors.astype(numpy.float32).astype(numpy.float64)
    err_g, err_s = _grad_error(on["grad"], f[:, None] * grad, S, n)
    X, V, hist = X0.copy(), numpy.zeros_like(X0), []
    for _ in range(k):
        Sk, _, gk = am.objective(X, terms, 0, "float32")
        hist.append(Sk)
        V = -lr * f[:, None] * gk
        X = X + V
    err_h = float(numpy.abs(on["hist", 0.0] / numpy.array(hist) - 1).max())
    err_x = float(numpy.abs(on["X", 0.0] - X).max() / numpy.abs(X).max())
    _report("anchored fit, 8 landmarks", info, gradient=err_g, stress=err_s, history=err_h, coordinates=err_x)
    assert err_g <= TOL and err_s <= TOL and err_h <= TOL and err_x <= TOL


def _peer_map():
    return _maps_d(DENSE_D, "pattern")[0]


def _set_peer_wish(eng):
    eng.set_wish_dense(_peer_map(), "wish", 1.0)
    return eng.stream_info()


def _stream_info(eng):
    return eng.stream_info()


def test_peer_ranks_that_share_the_gpu_drop_the_stream(monkeypatch, start_d, _no_rank_process_outlives_its_test):
    """Two ranks, a process each, on the one GPU: before the connect a rank holds a stream, after it
    none (the packed sweep is built for a rank that has the GPU to itself) -- asserted BEFORE the
    first iteration, which is enqueued only if it holds.  Then the steps are the stream-off run's."""
    from tests import _ranks
    world, k = 2, 4
    monkeypatch.setenv("BB_PEER_TIMEOUT_MS", "5000")
    w = _peer_map()
    want = [pm.model(w, ND, *pm.rank_range(10 * UPT, r, world), 1)[0] for r in range(world)]

    def scenario(on):
        ranks = _ranks.start(world, ND, "float32")
        try:
            before = [r.run(_set_peer_wish) for r in ranks]
            n_local = [b["packed_units"] + b["raw_units"] for b in before]
            assert before == (want if on else [_no_stream(m) for m in n_local])
            _ranks.connect(ranks)
            after = [r.run(_stream_info) for r in ranks]
            # the guard, before anything is handed to the device
            assert after == [_no_stream(m) for m in n_local], \
                "ranks that share a GPU kept their 24-bit stream after the connect: not iterating"
            for r in ranks:
                r.set_coords(start_d)
                r.set_momentum(0.2)
            for r in ranks:
                r.iterate_peer(k, LR_D)
            out = {}
            for r in ranks:
                assert r.peer_status() == 0
                out["X", r.rank], out["hist", r.rank] = r.get_coords(), r.stress_history()
            return before[0], out
        finally:
            _ranks.close_all()

    (info, on), (_, off) = _twins(monkeypatch, {"BB_PACK24_MIN_RUN": 1}, scenario)
    assert info["packed_units"] > 0
    _assert_same_bits(on, off, "peer ranks")
    assert _same(on["X", 0], on["X", 1]) and on["hist", 0].shape == (k,)
    _report("two peer ranks on one GPU, before the connect", info)


def _iterate_dist_twins(_, x0, k):
    """In a rank process: k steps of bb_solver_iterate_dist at world 1, with the stream and without
    it.  The library's own communicator of one rank (nobody to carry its id to) is made once; the
    library keeps it for the process and the second engine borrows it."""
    import os
    out = []
    for flag in (1, 0):
        os.environ["BB_PACK24"] = str(flag)
        eng = HipEngine(ND, "float32")
        try:
            eng.set_wish_dense(_peer_map(), "wish", 1.0)
            info = eng.stream_info()
            if not (eng._comm_cached() and eng._comm_attach()):
                uid = ctypes.create_string_buffer(128)
                _lib.check(eng._lib.bb_comm_unique_id(uid), "bb_comm_unique_id")
                _lib.check(eng._lib.bb_solver_comm_init(eng._h, uid.raw), "bb_solver_comm_init")
            assert eng.comm_world() == 1
            eng.set_coords(x0)
            eng.set_momentum(0.5)
            eng.iterate_dist(k, LR_D)
            eng.sync()
            out.append((info, eng.traffic()["unit_bytes"], {"X": eng.get_coords(), "hist": eng.stress_history()}))
        finally:
            eng.close()
    return out


def test_iterate_dist_at_world_1(monkeypatch, start_d, maps_e, _no_rank_process_outlives_its_test):
    """bb_solver_iterate_dist's loop (grad, the library's all-reduce, apply) at world 1, in a process
    of its own: a collective library's communicator is made in a fresh process, as a job makes it."""
    from tests import _ranks
    k = 5
    want = pm.model(maps_e[0], ND, 0, 10 * UPT, 1)[0]
    _env(monkeypatch, BB_PACK24=1, BB_PACK24_MIN_RUN=1)
    rank = _ranks.start(1, ND, "float32")[0]
    (info, nbytes, on), (info_off, nbytes_off, off) = rank.run(_iterate_dist_twins, start_d, k)
    assert info == want and info["packed_units"] > 0 and nbytes == want["stream_bytes"]
    assert info_off == _no_stream(10 * UPT) and nbytes_off == 10 * UPT * 8192
    _assert_same_bits(on, off, "iterate_dist")
    X_ref, h_ref = pm.run(maps_e[0], ND, start_d, k, LR_D, mu=0.5)
    err_h = float(numpy.abs(on["hist"] / h_ref - 1).max())
    err_x = float(numpy.abs(on["X"] - X_ref).max() / numpy.abs(X_ref).max())
    _report("world 1 through iterate_dist", info, history=err_h, coordinates=err_x)
    assert on["hist"].shape == (k,) and err_h < TOL and err_x < TOL
