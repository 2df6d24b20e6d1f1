"""Helpers for the tests of several maps in one solver (StructureSolver.fit_many,
bb_solver_set_maps): Hi-C-like batches whose maps live at very different scales, the float64
model of every map's step (docs/SPEC.md 2.4 / 2.4.1), the oracle's run of one map alone, and
host-side restatements of two rules of the product -- where `_fit_many_local` puts the maps
(`joint_layout`) and which units `build_indices` gives each wave (`wave_plan`) -- from which
the tests show that the waves they launch do cross map boundaries.  No GPU is needed here;
tests/test_many_model_cpu.py checks this file, tests/test_gpu_fit_many.py uses it."""
import collections
import functools

import numpy

from blueberry_amd.utils import HG19_CHROM_SIZES
from tests import _oracle
from tests.test_gpu_weighted import _counts
from tests.test_weighted_stress import count_map, start, weights, wish_of

TOL = {"float64": 1e-12, "float32": 1e-5}
# what the device's pow may add to a wish distance made from a count (docs/SPEC.md 4)
POW_EXTRA = {"float64": 1e-12, "float32": 2.0 ** -21}
SMALL = 16                    # below: a complete map (one missing pair from 7 bins on)
F64_WIDE_FROM = 4096          # fp64: 128-wide tiles up to this many bins, 512-wide above
HIST_CAP = 1 << 20            # stress values a solver's history holds

# q: weight power; mu: momentum; degree_steps: a step per bin (SPEC 2.4.1)
Setting = collections.namedtuple("Setting", "q mu degree_steps")
Batch = collections.namedtuple("Batch", "sizes counts wish starts")

# ---- the batches ------------------------------------------------------------------------------
# every map exactly one block of the layout (n_maps == n_blocks): in fp64 the first is laid out
# in 128-wide tiles and the second in 512-wide ones; in fp32 both in 512-wide ones
ONE_BLOCK_NARROW = (128, 5, 100, 128, 64)
ONE_BLOCK_WIDE = (512, 100, 512, 2, 300, 512, 400, 512, 17, 512, 512, 450)

SIZE_EDGES = collections.OrderedDict([
    ("tiny", (2, 3, 5)),
    ("three_tiles", (512, 512, 512)),
    ("narrow_edges", (128, 256, 384, 127, 129)),
    ("two_bins_between", (513, 2, 640)),
    ("around_1024", (1024, 1023, 1025)),
    ("around_2048", (2049, 2048, 2047)),
    ("large_then_two", (3000, 2)),
    ("two_then_large", (2, 3000)),
    ("wide_4096_100", (4096, 100)),
    ("narrow_100_3900", (100, 3900)),
    ("twelve_of_700", (700,) * 12),
    ("forty_ragged", tuple(int(v) for v in numpy.random.default_rng(123).integers(2, 901, 40))),
    ("one_block_narrow", ONE_BLOCK_NARROW),
    ("one_block_wide", ONE_BLOCK_WIDE),
])
SPECTRAL = (2, 3, 5, 40)
# chr1 .. chr22 and chrX of hg19 at 1 Mb per bin: 49 to 250 bins
GENOME_1MB = tuple(-(-length // 1000000) for length in HG19_CHROM_SIZES[:23])
# single-tile maps for the waves that pass through whole maps: 2 .. 40 bins, a few that fill
# their tile to the last bin (the next map then abuts) or but one.  311 of them: with one wave
# per CU a wave then has more units than a tile on 256 CUs and on 304 (fp32 155 / 130 of 128,
# fp64 311 / 261 of 256) and the chunks do not line up with the tiles, so some wave holds the
# end of one map, the whole of the next and the beginning of a third (270 maps do that on 256
# CUs only; tests/test_many_model_cpu.py holds both)
_FULL = {5: 512, 6: 511, 100: 511, 101: 512, 102: 512, 200: 512, 310: 511}
THROUGH = tuple(_FULL.get(i, 2 + (i * 7) % 39) for i in range(311))
ISOLATION = {"fp32": ("float32", (512, 300, 512, 2, 512)),
             "fp64_narrow": ("float64", (512, 300, 512, 2, 512)),
             "fp64_wide": ("float64", (512, 300, 512, 2, 512, 1024, 1025))}
HISTORY = (2,) * 23


def map_scale(m):
    """What map m's coordinates and wish distances are multiplied by."""
    return 2.0 ** (m % 7)


def counts_of(n, seed, m=0):
    """Count map number m of a batch: Hi-C-like with a dead bin, missing pairs and a NaN and an
    inf entry (below 16 bins: complete, but for one pair from 7 bins on), its counts times
    map_scale(m)^-3 -- a power of two -- so that its wish distances c^(-1/3) are the unscaled
    map's times map_scale(m)."""
    c = _counts(n, seed) if n < SMALL else count_map(n, seed=seed, bad=2)
    return c * map_scale(m) ** -3.0


@functools.lru_cache(maxsize=2)
def _counts_of_batch(sizes, seed):
    return tuple(counts_of(n, seed + 101 * m + n, m) for m, n in enumerate(sizes))


@functools.lru_cache(maxsize=2)
def batch(sizes, seed, dtype="float64"):
    """Count maps, wish maps (rounded to `dtype`, as float64) and starts for a tuple of sizes."""
    sizes = tuple(int(n) for n in sizes)
    counts = _counts_of_batch(sizes, seed)
    wish = tuple(wish_of(c, dtype) for c in counts)
    starts = tuple(start(n, w, seed=seed + 7 + m) for m, (n, w) in enumerate(zip(sizes, wish)))
    return Batch(sizes, counts, wish, starts)


# ---- the model of one map's step and run --------------------------------------------------------
def steps(W, setting):
    """(lr, bin_scale or None) of SPEC 2.4 / 2.4.1 for one map with lr='auto', in float64."""
    n = W.shape[0]
    if setting.q == 0:
        if not setting.degree_steps:
            return 1.0 / (2.0 * n), None
        deg = (W > 0).sum(1)
        top = int(deg.max())
        return 1.0 / (2.0 * (top + 1)), (top + 1.0) / (deg + 1.0)
    s = weights(W, setting.q).sum(1)
    top = float(s.max())
    if top <= 0.0:
        return 1.0 / (2.0 * n), None
    scale = numpy.where(s > 0, top / numpy.where(s > 0, s, 1.0), 1.0) if setting.degree_steps else None
    return 1.0 / (2.0 * top), scale


def step_bound(W, setting, dtype):
    """The relative distance allowed between the solver's step of a map (lrs_) and steps()'s:
    0 where the step is made of integers, else what `_input_model.weight_sum_bound` allows the
    largest weighted degree (relative: the largest of bound_i / s_i bounds the maximum's error)
    and 2^-51 for the two divisions on either side."""
    if setting.q == 0:
        return 0.0
    from tests import _input_model as im
    s = im.weight_sums_of(W, setting.q)
    bound = im.weight_sum_bound(W, setting.q, POW_EXTRA[dtype])
    return float((bound[s > 0] / s[s > 0]).max()) + 2.0 ** -51


def reference(W, x0, k, setting, dtype):
    """The oracle's K steps on one map alone: (X_K, history, lr, bin_scale)."""
    lr, scale = steps(W, setting)
    X, h = _oracle.load().solve_weighted(W, x0, k, lr, setting.q, mu=setting.mu, bin_scale=scale,
                                         f64=dtype == "float64")
    return X, h, lr, scale


def errors(n, X, h, X_ref, h_ref, against=None):
    """(stress error, coordinate error) of one map, relative.  On every entry of the history;
    below 16 bins against the start's stress, because such a map can reach its wish distances
    exactly and its later stresses are then rounding noise.  `against`: what to measure such a
    map's stresses against where the start's own may be 0 too (a spectral start)."""
    assert h.shape == h_ref.shape and X.shape == X_ref.shape
    if n < SMALL:
        err_s = float(numpy.abs(h - h_ref).max() / (h_ref[0] if against is None else against)) if h.size else 0.0
    else:
        err_s = float(numpy.abs(h / h_ref - 1).max()) if h.size else 0.0
    return err_s, float(numpy.abs(X - X_ref).max() / numpy.abs(X_ref).max())


def collapsed_stress(W):
    """The sum of delta^2 over the constrained pairs: the stress of a structure with every bin in
    one point, the scale docs/SPEC.md 2.8 normalises a stress by."""
    return float((numpy.triu(W, 1) ** 2).sum())


# ---- where the maps lie and which wave sweeps what ------------------------------------------------
def tile_edge(total, dtype):
    return 512 if dtype != "float64" or total > F64_WIDE_FROM else 128


def joint_layout(sizes, dtype):
    """The layout `_fit_many_local` gives a batch: every map starts at a multiple of the tile
    edge (128 only while an fp64 batch laid out that way has at most 4,096 bins), and the tile
    list is every map's dense upper triangle, in device order (J, then I).  Returns a dict: off,
    total, vw, units_per_tile, n_blocks, tiles (I, J), tile_map (the map of every tile), n_units."""
    def lay(vw):
        off = [0]
        for n in sizes[:-1]:
            off.append(off[-1] + -(-n // vw) * vw)
        return off, off[-1] + sizes[-1]
    off, total = lay(128)
    if tile_edge(total, dtype) != 128:
        off, total = lay(512)
    vw = tile_edge(total, dtype)
    rows_per_unit = 4 if dtype != "float64" else (2 if vw == 512 else 8)
    ti, tj, tm = [], [], []
    for m, (o, n) in enumerate(zip(off, sizes)):
        b0, b1 = o // vw, -(-(o + n) // vw)
        for j in range(b0, b1):
            for i in range(b0, j + 1):
                ti.append(i)
                tj.append(j)
                tm.append(m)
    # (a map's blocks are a run and the maps ascend: this order is already J, then I)
    upt = vw // rows_per_unit
    return {"off": off, "total": total, "vw": vw, "units_per_tile": upt,
            "n_blocks": -(-total // vw),
            "tiles": (numpy.array(ti, dtype=numpy.int32), numpy.array(tj, dtype=numpy.int32)),
            "tile_map": numpy.array(tm, dtype=numpy.int64), "n_units": len(ti) * upt}


def launch_shape(n_units, dtype, vw, cus, waves_per_cu=None):
    """(waves per CU, waves per workgroup) of the sweep: 4 per CU below 65,000 units and 8 from
    there on unless BB_WAVES_PER_CU says otherwise (1 .. 32); workgroups of 8 waves with 8 or
    more per CU on the 512-wide layouts, else of 4."""
    wpc = (8 if n_units >= 65000 else 4) if waves_per_cu is None else min(32, max(1, int(waves_per_cu)))
    wide = dtype != "float64" or vw == 512
    nw = max(1, min(cus * wpc, n_units))
    return wpc, (8 if wide and wpc >= 8 and nw >= 8 else 4)


def wave_plan(n_units, units_per_tile, tile_map, cus, waves_per_cu, wpb):
    """The chunk rule of the sweep: nw = round_up(min(cus * wpc, n_units), wpb) waves, wave w
    owning the units [w q + min(w, r), + q (+ 1 if w < r)), q, r = divmod(n_units, nw).  Returns,
    per wave, the maps its units belong to, in sweep order (empty: a wave without units)."""
    nw = max(1, min(cus * waves_per_cu, n_units))
    nw = -(-nw // wpb) * wpb
    q, r = divmod(n_units, nw)
    plan = []
    for w in range(nw):
        a = w * q + min(w, r)
        b = a + q + (1 if w < r else 0)
        if a >= b:
            plan.append([])
            continue
        maps = tile_map[a // units_per_tile:(b - 1) // units_per_tile + 1]
        keep = numpy.concatenate([[True], maps[1:] != maps[:-1]])
        plan.append([int(m) for m in maps[keep]])
    return plan


def crossing(plan):
    """(waves that hold units of two maps or more, the most maps one wave holds, waves with units)."""
    held = [len(p) for p in plan if p]
    return sum(1 for v in held if v >= 2), max(held), len(held)
