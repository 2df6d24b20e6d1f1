"""CPU: the sweep plan and the 24-bit stream's table as the library computes them
(bb_layout_sweep_plan, bb_layout_pk24_table: the host arithmetic behind bb_solver_create and
ensure_pk24, csrc/bb_solver_plan.cpp) against an independent statement of docs/SPEC.md 3.3-3.7 in
Python: tests/_pack24_model.py for the chunks, the run rule and the table, and the properties every
slot, reduce list and LDS size must have for the kernels that index with them to stay in bounds.
No device is touched.  Not tested: the refusal of a stream of 2^31 KiB or more (pk24_table's
`pays`), which needs about 2^28 units."""
import ctypes

import numpy
import pytest

from blueberry_amd import _lib
from tests import _pack24_model as pm

F32, F64 = _lib.BB_F32, _lib.BB_F64
LDS_PER_CU = 160 * 1024


def layout(n_bins, dtype):
    """SPEC 3.1: tile edge, rows per unit, units per tile, blocks; the narrow fp64 shape up to 4,096 bins."""
    wide = dtype == F32 or n_bins > 4096
    vw = 512 if wide else 128
    rpu = 4 if dtype == F32 else (2 if wide else 8)
    return {"wide": wide, "vw": vw, "rpu": rpu, "upt": vw // rpu, "nb": -(-n_bins // vw),
            "es": 4 if dtype == F32 else 8}


def dense_tiles(nb):
    I = numpy.array([i for j in range(nb) for i in range(j + 1)], dtype=numpy.int32)
    J = numpy.array([j for j in range(nb) for i in range(j + 1)], dtype=numpy.int32)
    return I, J


def band_tiles(nb, width=1):
    I, J = dense_tiles(nb)
    keep = J - I <= width
    return I[keep], J[keep]


def _ptr(a, ctype):
    return a.ctypes.data_as(ctypes.POINTER(ctype))


def plan(n_bins, dtype, tiles, u_begin, u_end, cus, wpc=0, pair=True, slices=0, row_owner=False):
    """The library's plan: its scalars as a dict, with the five arrays under their names."""
    lib = _lib.load()
    knobs = _lib.SweepKnobs(wpc, int(pair), slices, int(row_owner))
    out = _lib.SweepPlan()
    none32, none64 = ctypes.POINTER(ctypes.c_int32)(), ctypes.POINTER(ctypes.c_int64)()
    if tiles is None:
        targs = (none32, none32, 0)
    else:
        I = numpy.ascontiguousarray(tiles[0], dtype=numpy.int32)
        J = numpy.ascontiguousarray(tiles[1], dtype=numpy.int32)
        targs = (_ptr(I, ctypes.c_int32), _ptr(J, ctypes.c_int32), I.size)
    # a call with NULL arrays returns the counts
    args = (n_bins, dtype) + targs + (u_begin, u_end, cus, ctypes.byref(knobs), ctypes.byref(out))
    _lib.check(lib.bb_layout_sweep_plan(*args, none32, none32, none32, none32, none64), "sweep_plan")
    p = out.as_dict()
    udesc = numpy.full((max(p["n_local"], 1), 2), -7, dtype=numpy.int32)
    wave_slots = numpy.full((p["n_waves"], 2), -7, dtype=numpy.int32)
    slot_strip = numpy.full(max(p["n_slots"], 1), -7, dtype=numpy.int32)
    wave_last = numpy.full(p["n_waves"], -7, dtype=numpy.int32)
    red = numpy.full((p["red_blocks"], p["red_stride"]), -7, dtype=numpy.int64)
    _lib.check(lib.bb_layout_sweep_plan(*args, _ptr(udesc, ctypes.c_int32), _ptr(wave_slots, ctypes.c_int32),
                                        _ptr(slot_strip, ctypes.c_int32), _ptr(wave_last, ctypes.c_int32),
                                        _ptr(red, ctypes.c_int64)), "sweep_plan")
    assert out.as_dict() == p
    p.update(udesc=udesc[:p["n_local"]], wave_slots=wave_slots, slot_strip=slot_strip[:p["n_slots"]],
             wave_last_strip=wave_last, red_lists=red)
    return p


def check_plan(n_bins, dtype, tiles, u_begin, u_end, cus, wpc=0, pair=True):
    """Everything that must hold of one plan; returns it."""
    L = layout(n_bins, dtype)
    vw, rpu, upt, ch = L["vw"], L["rpu"], L["upt"], 3 * L["vw"]
    I, J = dense_tiles(L["nb"]) if tiles is None else tiles
    I, J = numpy.asarray(I, dtype=numpy.int64), numpy.asarray(J, dtype=numpy.int64)
    p = plan(n_bins, dtype, tiles, u_begin, u_end, cus, wpc, pair)
    n_local = u_end - u_begin
    assert p["n_local"] == n_local
    assert p["red_blocks"] == L["nb"]

    # the units: SPEC 3.2
    u = numpy.arange(u_begin, u_end)
    assert numpy.array_equal(p["udesc"][:, 0], I[u // upt] * vw + (u % upt) * rpu)
    assert numpy.array_equal(p["udesc"][:, 1], J[u // upt] * vw)
    strips = J[u // upt]
    t_first = u_begin // upt if n_local else 0
    n_tiles = (u_end - 1) // upt - t_first + 1 if n_local else 0
    assert (p["t_first"], p["n_local_tiles"]) == (t_first, n_tiles)

    # the waves: SPEC 3.3, as tests/_pack24_model.py states it
    rule_wpc = wpc if wpc else (8 if n_local >= 65000 else 4)
    wpb = pm.waves_per_block(n_local, cus, rule_wpc, pair) if L["wide"] else 4
    assert p["wpb"] == wpb
    chunks = pm.chunks(n_local, cus, rule_wpc, wpb)
    nw = len(chunks)
    assert p["n_waves"] == nw and nw % wpb == 0
    q, r = p["chunk_q"], p["chunk_r"]
    mine = [(w * q + min(w, r), w * q + min(w, r) + q + (1 if w < r else 0)) for w in range(nw)]
    assert mine == chunks
    assert chunks[0][0] == 0 and chunks[-1][1] == n_local          # they tile [0, n_local) exactly
    assert all(chunks[w][1] == chunks[w + 1][0] for w in range(nw - 1))

    # column-partial slots
    ws, slot_strip = p["wave_slots"], p["slot_strip"]
    used = numpy.zeros(p["n_slots"], dtype=int)
    owner = {}                     # shared slot -> (workgroup, strip) of the waves that end in it
    for w, (a, b) in enumerate(chunks):
        x, y = int(ws[w, 0]), int(ws[w, 1])
        if a == b:
            assert y == -1 and p["wave_last_strip"][w] == -1
            continue
        s = strips[a:b]
        distinct = s[numpy.r_[True, s[1:] != s[:-1]]]
        k = distinct.size - 1
        assert 0 <= x and x + k <= p["n_slots"] and 0 <= y < p["n_slots"]
        assert numpy.array_equal(slot_strip[x:x + k], distinct[:-1])          # private, consecutive
        used[x:x + k] += 1
        assert slot_strip[y] == distinct[-1] == p["wave_last_strip"][w]
        assert not (x <= y < x + k)
        assert owner.setdefault(y, (w // wpb, int(distinct[-1]))) == (w // wpb, int(distinct[-1]))
    assert (used[sorted(owner)] == 0).all()                                   # a shared slot is nobody's private one
    used[sorted(owner)] += 1
    assert (used == 1).all()                                                  # every slot is referenced, once
    assert p["rowpart_elems"] == n_tiles * ch and p["colpart_elems"] == p["n_slots"] * ch
    assert p["zero_off"] == p["rowpart_elems"] + p["colpart_elems"]
    assert p["part_total"] == p["zero_off"] + ch

    # reduce lists: block b <- the row chunks of its local tiles, then the column slots of strip b
    red, stride, slices = p["red_lists"], p["red_stride"], p["red_slices"]
    local_I = I[t_first:t_first + n_tiles]
    longest, seen = 0, []
    for b in range(L["nb"]):
        want = [int(lt) * ch for lt in numpy.nonzero(local_I == b)[0]]
        want += [p["rowpart_elems"] + int(sl) * ch for sl in numpy.nonzero(slot_strip == b)[0]]
        assert red[b, :len(want)].tolist() == want
        assert (red[b, len(want):] == p["zero_off"]).all()                    # padding: the chunk of zeros
        longest = max(longest, len(want))
        seen += want
    assert len(seen) == len(set(seen)) == n_tiles + p["n_slots"]              # each entry once overall
    assert slices == (4 if longest <= 64 else 8)
    assert stride % (16 * slices) == 0 and longest <= stride < max(longest, 1) + 16 * slices
    assert red.min() >= 0 and red.max() + ch <= p["part_total"]

    # LDS of the sweep
    assert p["defer_lds_bytes"] == wpb * p["lds_wave_floats"] * 4 + 32
    assert p["lds_wave_floats"] * 4 >= ch * L["es"]                           # a column partial fits
    assert p["lds_wave_floats"] >= p["defer_cap_units"] * 12                  # and 12 words per parked unit
    wgs_per_cu = max(1, -(-(nw // wpb) // cus))
    assert wgs_per_cu * p["defer_lds_bytes"] <= LDS_PER_CU
    assert (p["defer_cap_units"] == 0) == (not L["wide"] or n_local == 0)
    assert p["defer_cap_units"] <= max(b - a for a, b in chunks)
    assert p["nontemporal"] == int(n_local * 8192 > 240 << 20)
    assert (p["full_ld"], p["ro_wpr"], p["ro_blocks"]) == (0, 1, 0)           # no row-owner knob
    return p


DENSE = [(F32, 2), (F32, 513), (F32, 4097), (F64, 2), (F64, 513), (F64, 4096), (F64, 4097)]


@pytest.mark.parametrize("dtype,n_bins", DENSE)
@pytest.mark.parametrize("world", [1, 2, 8])
def test_dense_lists_every_rank(dtype, n_bins, world):
    """The three layouts on either side of the fp64 switch (4,096 | 4,097 bins), every rank of
    worlds 1, 2 and 8: ranges that begin and end inside a tile, and ranks without a unit."""
    L = layout(n_bins, dtype)
    n_units = L["nb"] * (L["nb"] + 1) // 2 * L["upt"]
    for rank in range(world):
        a, b = pm.rank_range(n_units, rank, world)
        for cus in (256, 4):
            check_plan(n_bins, dtype, None, a, b, cus)


@pytest.mark.parametrize("world,rank", [(1, 0), (2, 1), (8, 0), (8, 3), (8, 7)])
def test_dense_24926(world, rank):
    """chr1 at 10 kb, fp32: 156,800 units; one rank holds them past the 65,000-unit rule (8 waves
    per CU, paired workgroups), a half still streams past the 240 MiB the cache keeps (non-temporal
    loads), an eighth does neither."""
    n_bins = 24926
    a, b = pm.rank_range(49 * 50 // 2 * pm.UPT, rank, world)
    p = check_plan(n_bins, F32, None, a, b, 256)
    assert p["wpb"] == (8 if b - a >= 65000 else 4)
    assert p["nontemporal"] == (1 if world < 8 else 0)         # 612 MiB a half, 153 MiB an eighth


@pytest.mark.parametrize("cus", [256, 4])
@pytest.mark.parametrize("dtype", [F32, F64])
def test_unit_counts_at_the_edges(dtype, cus):
    """n_local of 0, 1, wpb - 1, cus * 4 +- 1 and 64,999 | 65,000, from a unit inside a tile."""
    n_bins = 24926
    u0 = 3 * layout(n_bins, dtype)["upt"] + 5
    for n_local in (0, 1, 3, 7, cus * 4 - 1, cus * 4, cus * 4 + 1, 64999, 65000):
        p = check_plan(n_bins, dtype, None, u0, u0 + n_local, cus)
        assert p["n_waves"] >= 4
        assert p["wpb"] == (8 if n_local >= 65000 else 4)


@pytest.mark.parametrize("pair", [True, False])
@pytest.mark.parametrize("wpc", [1, 4, 8])
def test_knobs(wpc, pair):
    """Waves per CU 1, 4 and 8, pairing on and off, on 256 CUs and on 4 -- where 8 unpaired waves
    per CU put two workgroups on a CU, which then share its LDS."""
    for dtype, n_bins in ((F32, 4097), (F64, 4097), (F64, 4096)):
        L = layout(n_bins, dtype)
        n_units = L["nb"] * (L["nb"] + 1) // 2 * L["upt"]
        for cus in (256, 4):
            p = check_plan(n_bins, dtype, None, 7, n_units - 3, cus, wpc, pair)
            assert p["wpb"] == (8 if pair and wpc == 8 and L["wide"] else 4)
            assert p["n_waves"] == -(-cus * wpc // p["wpb"]) * p["wpb"]
    p = check_plan(4097, F32, None, 0, 45 * pm.UPT, 4, 8, False)
    assert p["n_waves"] // p["wpb"] == 8 and 2 * p["defer_lds_bytes"] <= LDS_PER_CU   # two workgroups per CU


def test_banded_list_chunks_cross_strips():
    """A band of two tiles per strip: on 4 CUs with one wave each a chunk runs through a dozen
    strips, all but the last with a private slot; and the same list cut among 8 ranks."""
    n_bins = 24926
    tiles = band_tiles(49)
    n_units = tiles[0].size * pm.UPT
    p = check_plan(n_bins, F32, tiles, 0, n_units, 4, 1)
    privates = p["wave_slots"][1:, 0] - p["wave_slots"][:-1, 0]
    assert p["n_waves"] == 4 and privates.min() >= 10
    for rank in range(8):
        a, b = pm.rank_range(n_units, rank, 8)
        check_plan(n_bins, F32, tiles, a, b, 256)
    # the narrow fp64 shape: 16 units per tile, so chunks cross strips on any machine
    tiles = band_tiles(32, 2)
    check_plan(4096, F64, tiles, 5, tiles[0].size * 16 - 9, 4, 1)
    check_plan(4096, F64, pm.map_tiles(tiles, [0, 1024, 4096], 1), 0, 200, 256)


def test_empty_tile_list():
    empty = (numpy.zeros(0, dtype=numpy.int32), numpy.zeros(0, dtype=numpy.int32))
    for dtype, n_bins in ((F32, 513), (F64, 513), (F64, 4097)):
        p = check_plan(n_bins, dtype, empty, 0, 0, 256)
        assert p["n_slots"] == 0 and p["n_waves"] == 4 and (p["wave_slots"][:, 1] == -1).all()
        assert (p["red_lists"] == p["zero_off"]).all() and p["part_total"] == 3 * layout(n_bins, dtype)["vw"]


def test_row_owner_sizes_and_reduce_slices_knob():
    for dtype, n_bins, ld, wpr in ((F32, 963, 1024, 4), (F64, 963, 1024, 4), (F32, 1025, 1280, 2),
                                   (F64, 2049, 2176, 1), (F32, 4096, 4096, 1)):
        L = layout(n_bins, dtype)
        n_units = L["nb"] * (L["nb"] + 1) // 2 * L["upt"]
        p = plan(n_bins, dtype, None, 0, n_units, 256, row_owner=True)
        assert p["full_ld"] == ld and ld % (256 if dtype == F32 else 128) == 0 and ld >= n_bins
        assert p["ro_wpr"] == wpr and p["ro_blocks"] == -(-n_bins // (4 // wpr))
    for slices in (4, 8):
        p = plan(4097, F32, None, 0, 45 * pm.UPT, 256, slices=slices)
        assert p["red_slices"] == slices and p["red_stride"] % (16 * slices) == 0


def test_refusals():
    lib = _lib.load()
    knobs, out = _lib.SweepKnobs(0, 1, 0, 0), _lib.SweepPlan()
    none32, none64 = ctypes.POINTER(ctypes.c_int32)(), ctypes.POINTER(ctypes.c_int64)()
    call = lambda a, b, cus: lib.bb_layout_sweep_plan(513, F32, none32, none32, 0, a, b, cus, ctypes.byref(knobs),
                                                      ctypes.byref(out), none32, none32, none32, none32, none64)
    assert call(0, 3 * pm.UPT, 256) == _lib.BB_OK
    assert call(0, 3 * pm.UPT + 1, 256) == _lib.BB_ERR_INVALID and "u_end" in _lib.last_error()
    assert call(5, 4, 256) == _lib.BB_ERR_INVALID
    assert call(0, 1, 0) == _lib.BB_ERR_INVALID and "cus" in _lib.last_error()
    I, J = numpy.array([0, 0], dtype=numpy.int32), numpy.array([1, 0], dtype=numpy.int32)   # not (J, I) ordered
    rc = lib.bb_layout_sweep_plan(1025, F32, _ptr(I, ctypes.c_int32), _ptr(J, ctypes.c_int32), 2, 0, 1, 256,
                                  ctypes.byref(knobs), ctypes.byref(out), none32, none32, none32, none32, none64)
    assert rc == _lib.BB_ERR_INVALID and "ordered" in _lib.last_error()


# ---- the 24-bit stream's table ---------------------------------------------------------------------
def pk24(lo, hi, min_run, mode):
    lib = _lib.load()
    n = len(lo)
    mm = numpy.ascontiguousarray(numpy.stack([lo, hi], 1), dtype=numpy.uint32).reshape(n, 2)
    udesc = numpy.stack([4 * numpy.arange(n), 512 * (numpy.arange(n) // 128)], 1).astype(numpy.int32)
    table = numpy.full((n, 4), -7, dtype=numpy.int32)
    kib, packed, switches = ctypes.c_int64(-1), ctypes.c_int64(-1), ctypes.c_int64(-1)
    pays = ctypes.c_int(-1)
    counts = (ctypes.byref(kib), ctypes.byref(packed), ctypes.byref(switches), ctypes.byref(pays))
    args = (_ptr(mm, ctypes.c_uint32), _ptr(udesc, ctypes.c_int32), n, min_run, mode)
    _lib.check(lib.bb_layout_pk24_table(*args, ctypes.POINTER(ctypes.c_int32)(), *counts), "pk24_table")
    first = (kib.value, packed.value, switches.value, pays.value)
    _lib.check(lib.bb_layout_pk24_table(*args, _ptr(table, ctypes.c_int32), *counts), "pk24_table")
    assert first == (kib.value, packed.value, switches.value, pays.value)
    assert numpy.array_equal(table[:, :2], udesc)
    z = table[:, 2].astype(numpy.int64) & 0xffffffff
    return {"offset_kib": z & 0x7fffffff, "packed": (z >> 31).astype(bool),
            "base": table[:, 3].astype(numpy.int64) & 0xffffffff,
            "kib": kib.value, "packed_units": packed.value, "switches": switches.value, "pays": pays.value}


def check_pk24(lo, hi, min_run, mode=-1):
    lo, hi = numpy.asarray(lo, dtype=numpy.int64), numpy.asarray(hi, dtype=numpy.int64)
    got = pk24(lo, hi, min_run, mode)
    packed = pm.run_rule(hi - lo < pm.SPAN, min_run)
    info, table = pm.describe(packed, lo)
    for key in ("offset_kib", "packed", "base"):
        assert numpy.array_equal(got[key], table[key]), key
    kib = int(numpy.where(packed, pm.PACKED_KIB, pm.RAW_KIB).sum())
    assert got["kib"] == kib and got["packed_units"] == int(packed.sum())
    assert got["switches"] == int((packed[1:] != packed[:-1]).sum())
    if info["packed_units"]:
        assert (info["stream_bytes"], info["format_switches"]) == (1024 * got["kib"], got["switches"])
    # mode 0 never, 1 whenever a unit is packed, else: the stream saves an eighth of the raw bytes
    raw_kib = pm.RAW_KIB * lo.size
    want = {0: False, 1: bool(packed.any())}.get(mode, lo.size > 0 and 8 * kib <= 7 * raw_kib)
    assert got["pays"] == int(want)
    return got


ONE, WIDE = 0x3f800000, 0x3f800000 + pm.SPAN       # a packable unit's words: [ONE, WIDE); WIDE - ONE is too far


def planted(runs):
    """(lo, hi) of units in runs of (length, packable)."""
    lo, hi = [], []
    for k, (length, packable) in enumerate(runs):
        lo += [ONE + k] * length
        hi += [(WIDE - 1 if packable else WIDE) + k] * length
    return lo, hi


@pytest.mark.parametrize("mode", [0, 1, -1])
@pytest.mark.parametrize("min_run", [1, 5, 64])
def test_pk24_runs_around_min_run(min_run, mode):
    """Runs of min_run - 1, min_run and min_run + 1 packable units between raw ones, a run at
    each end of the range, and the span boundary 2^24 - 1 | 2^24."""
    runs = [(min_run + 1, True), (3, False), (max(min_run - 1, 1), True), (2, False), (min_run, True),
            (1, False), (min_run, True)]
    got = check_pk24(*planted(runs), min_run, mode)
    assert got["packed"][0] and got["packed"][-1]
    assert got["packed"][min_run + 4] == (min_run == 1)
    got = check_pk24(*planted([(2, False), (min_run, True), (2, False)]), min_run, mode)
    assert not got["packed"][0] and not got["packed"][-1] and got["packed"][2]
    check_pk24(*planted([(min_run - 1, True)] if min_run > 1 else [(1, False)]), min_run, mode)
    check_pk24([], [], min_run, mode)


def test_pk24_zero_unit_inside_a_packed_run():
    lo, hi = planted([(70, True)])
    lo[30] = hi[30] = 0                               # an all-zero unit: packable, base 0
    got = check_pk24(lo, hi, 64)
    assert got["packed"].all() and got["base"][30] == 0 and got["base"][29] == ONE


def test_pk24_saving_threshold():
    """p of n units packed: the stream is 8 n - 2 p KiB and pays from p = n / 2 on."""
    for n, p, pays in ((8, 4, 1), (8, 3, 0), (64, 32, 1), (64, 31, 0)):
        for mode in (-1, 1, 0):
            got = check_pk24(*planted([(p, True), (n - p, False)]), 1, mode)
            assert got["pays"] == (pays if mode == -1 else mode)
