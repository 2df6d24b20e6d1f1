"""No GPU: the helpers of tests/_many_model.py hold what tests/test_gpu_fit_many.py relies on --
the batches stay well above rounding noise under the oracle, `joint_layout` is the layout
`_fit_many_local` hands its engine, the steps it folds into the per-bin factors are the model's,
and `wave_plan` gives the waves of tests 2 and 3 units of more than one map on a chip of 256
compute units and on one of 304."""
import numpy
import pytest

import blueberry_amd as bb
from blueberry_amd.solver import layout_info
from tests import _many_model as mm
from tests.test_weighted_stress import weights, wish_of

EDGE_SETTINGS = [mm.Setting(0, 0.0, False), mm.Setting(0, 0.3, False), mm.Setting(1, 0.0, False),
                 mm.Setting(2, 0.0, False)]
GENOME_SETTINGS = [mm.Setting(q, 0.0, d) for q in (0, 1, 2) for d in (False, True)]


def _floor(sizes, seed, k, settings):
    """The smallest h.min() / h[0] over the maps of at least 16 bins and the settings."""
    b = mm.batch(tuple(sizes), seed)
    worst = numpy.inf
    for m, n in enumerate(b.sizes):
        if n < mm.SMALL:
            continue
        for s in settings:
            _, h, _, _ = mm.reference(b.wish[m], b.starts[m], k, s, "float64")
            assert numpy.isfinite(h).all() and (h > 0).all()
            worst = min(worst, float(h.min() / h[0]))
    return worst


@pytest.mark.parametrize("name", [k for k, v in mm.SIZE_EDGES.items() if max(v) >= mm.SMALL])
def test_size_edge_batches_stay_above_noise(name):
    """The entry-wise relative tolerance is not measured on noise: no map's stress falls below
    a thousandth of its start's in the K = 4 steps of the test."""
    assert _floor(mm.SIZE_EDGES[name], 1, 4, EDGE_SETTINGS) >= 1e-3


def test_other_batches_stay_above_noise():
    assert _floor(mm.GENOME_1MB, 2, 6, GENOME_SETTINGS) >= 1e-3
    assert _floor(mm.THROUGH, 3, 3, [mm.Setting(0, 0.0, False), mm.Setting(2, 0.0, False)]) >= 1e-3
    assert _floor(mm.SPECTRAL, 4, 2, EDGE_SETTINGS[:1]) >= 1e-3


def test_batches_are_what_the_tests_say():
    assert len(mm.GENOME_1MB) == 23 and min(mm.GENOME_1MB) == 49 and max(mm.GENOME_1MB) == 250
    assert len(mm.SIZE_EDGES["forty_ragged"]) == 40
    assert 2 <= min(mm.SIZE_EDGES["forty_ragged"]) and max(mm.SIZE_EDGES["forty_ragged"]) <= 900
    assert max(mm.THROUGH) == 512 and min(mm.THROUGH) == 2
    assert sorted(set(mm.THROUGH) - set(range(2, 41))) == [511, 512]
    b = mm.batch((40, 60, 5, 9), 0)
    for m, (n, c, w) in enumerate(zip(b.sizes, b.counts, b.wish)):
        assert c.shape == w.shape == (n, n) and numpy.array_equal(w, w.T)
        if n >= mm.SMALL:
            assert (w == 0).all(axis=1).any()                  # a dead bin
            assert numpy.isnan(c).any() and numpy.isinf(c).any()
        assert (w[numpy.triu_indices(n, 1)] == 0).any() == (n >= 7)   # a missing pair
        # map m lives at 2^(m % 7) times the scale of the same map as number 0
        plain = wish_of(c * mm.map_scale(m) ** 3.0, "float64")
        assert numpy.abs(w - mm.map_scale(m) * plain).max() <= 4e-16 * w.max()


# ---- joint_layout is _fit_many_local's ------------------------------------------------------------
class _Recorder(object):
    """An engine that records what fit_many hands it and answers the probes from the model."""
    made = []

    def __init__(self, n_bins, dtype, rank=0, world=1, device=0, tiles=None):
        self.n_bins, self.dtype, self.tiles, self.q = n_bins, dtype, tiles, 0
        self.w = None                     # the joint wish matrix, once a map has an entry
        self.steps = None
        _Recorder.made.append(self)

    def set_maps(self, bin_begin, lr_scale):
        self.bin_begin, self.lr_scale = list(bin_begin), list(lr_scale)

    def set_wish_dense_block(self, matrix, bin_offset, kind, alpha):
        n = matrix.shape[0]
        assert kind == "counts"
        if not numpy.asarray(matrix).any():
            return
        if self.w is None:
            self.w = numpy.zeros((self.n_bins, self.n_bins))
        self.w[bin_offset:bin_offset + n, bin_offset:bin_offset + n] = wish_of(matrix, self.dtype, alpha)

    def set_weight_power(self, q):
        self.q = q

    def weight_sums(self):
        return weights(self.w, self.q).sum(1)

    def degrees(self):
        return (self.w > 0).sum(1).astype(numpy.int64)

    def set_bin_steps(self, scale):
        self.steps = numpy.array(scale)

    def set_coords(self, x0):
        self.x0 = numpy.array(x0)

    def iterate(self, iters, lr):
        self.lr = lr

    def get_coords(self):
        return self.x0

    def stress_history(self):
        return numpy.zeros(0)

    def close(self):
        pass


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("sizes", [mm.SIZE_EDGES["narrow_edges"], mm.SIZE_EDGES["two_bins_between"],
                                   mm.SIZE_EDGES["wide_4096_100"], mm.SIZE_EDGES["narrow_100_3900"],
                                   mm.ONE_BLOCK_NARROW, mm.ONE_BLOCK_WIDE, mm.GENOME_1MB,
                                   mm.ISOLATION["fp64_wide"][1]])
def test_joint_layout_is_the_one_fit_many_makes(sizes, dtype):
    lay = mm.joint_layout(sizes, dtype)
    info = layout_info(lay["total"], dtype)
    assert (lay["vw"], lay["units_per_tile"], lay["n_blocks"]) == (
        info["vw"], info["units_per_tile"], info["n_blocks"])
    zeros = [numpy.zeros((n, n)) for n in sizes]
    bb.StructureSolver(n_iter=1, dtype=dtype, engine=_Recorder).fit_many(zeros)
    eng = _Recorder.made.pop()
    assert eng.n_bins == lay["total"] and eng.bin_begin == lay["off"] + [lay["total"]]
    assert numpy.array_equal(eng.tiles[0], lay["tiles"][0])
    assert numpy.array_equal(eng.tiles[1], lay["tiles"][1])
    assert lay["n_units"] == len(lay["tiles"][0]) * lay["units_per_tile"]
    # every tile lies within one map, and the tile_map says which
    begin = numpy.array(lay["off"])
    for k in (0, 1):
        assert numpy.array_equal(numpy.searchsorted(begin, lay["tiles"][k] * lay["vw"], side="right") - 1,
                                 lay["tile_map"])


def test_one_block_batches_have_a_map_per_block():
    for dtype, sizes, vw in (("float64", mm.ONE_BLOCK_NARROW, 128), ("float64", mm.ONE_BLOCK_WIDE, 512),
                             ("float32", mm.ONE_BLOCK_NARROW, 512), ("float32", mm.ONE_BLOCK_WIDE, 512)):
        lay = mm.joint_layout(sizes, dtype)
        assert lay["vw"] == vw and lay["n_blocks"] == len(sizes) == len(lay["tiles"][0])
    for name, (dtype, sizes) in mm.ISOLATION.items():
        lay = mm.joint_layout(sizes, dtype)
        assert lay["vw"] == (128 if name == "fp64_narrow" else 512)
        # maps 0 | 1 and 2 | 3 abut: no padding row between them
        assert lay["off"][1] == sizes[0] and lay["off"][3] == lay["off"][2] + sizes[2]


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("setting", [mm.Setting(0, 0.0, True), mm.Setting(1, 0.0, False),
                                     mm.Setting(2, 0.0, False), mm.Setting(2, 0.0, True)])
def test_fit_many_folds_the_models_steps_into_the_bin_factors(setting, dtype):
    """With weight_power or degree_steps every map's whole step reaches the update through the
    per-bin factors and the solver iterates with lr = 1: factor of bin i of map m = the model's
    lr_m * scale_m[i] (a few roundings apart: the product multiplies before it divides), 1 on
    the padding, lrs_[m] the model's lr_m."""
    b = mm.batch((40, 130, 5, 70), 5, dtype)
    s = bb.StructureSolver(n_iter=1, dtype=dtype, engine=_Recorder, weight_power=setting.q,
                           degree_steps=setting.degree_steps).fit_many(list(b.counts), inits=list(b.starts))
    eng = _Recorder.made.pop()
    lay = mm.joint_layout(b.sizes, dtype)
    assert eng.lr == 1.0 and eng.steps.shape == (lay["total"],)
    covered = numpy.zeros(lay["total"], dtype=bool)
    for m, (o, n) in enumerate(zip(lay["off"], b.sizes)):
        lr, scale = mm.steps(b.wish[m], setting)
        want = lr * (numpy.ones(n) if scale is None else scale)
        assert numpy.abs(eng.steps[o:o + n] / want - 1).max() <= 2.0 ** -50
        assert abs(s.lrs_[m] / lr - 1) <= (0.0 if setting.q == 0 else 2.0 ** -50)
        assert numpy.array_equal(eng.x0[o:o + n], b.starts[m])
        covered[o:o + n] = True
    assert (eng.steps[~covered] == 1.0).all() and not eng.x0[~covered].any()


# ---- wave_plan -------------------------------------------------------------------------------------
def test_wave_plan_is_the_chunk_rule():
    tile_map = numpy.array([0, 0, 0, 1, 2, 2])
    # 24 units in tiles of 4, 2 CUs x 3 waves -> 6 waves rounded up to 8: 3 units each
    plan = mm.wave_plan(24, 4, tile_map, 2, 3, 4)
    assert plan == [[0], [0], [0], [0], [1], [1, 2], [2], [2]]
    assert mm.crossing(plan) == (1, 2, 8)
    # 22 units, 8 waves: q = 2, r = 6 -- six waves of 3 units, then [18, 20) and [20, 22)
    assert mm.wave_plan(22, 4, tile_map, 2, 4, 4) == plan
    # 5 waves: q = 4, r = 4 -- [0, 5) [5, 10) [10, 15) [15, 20) [20, 24)
    plan = mm.wave_plan(24, 4, tile_map, 5, 1, 1)
    assert plan == [[0], [0], [0, 1], [1, 2], [2]]
    assert mm.crossing(plan) == (2, 2, 5)
    # fewer units than waves: 3 units -> 3 waves rounded up to 4, the last without units
    assert mm.wave_plan(3, 1, numpy.array([0, 1, 1]), 256, 4, 4) == [[0], [1], [1], []]
    # one wave through everything
    assert mm.wave_plan(24, 4, tile_map, 1, 1, 1) == [[0, 1, 2]]
    assert mm.launch_shape(2944, "float32", 512, 256) == (4, 4)
    assert mm.launch_shape(70000, "float32", 512, 256) == (8, 8)
    assert mm.launch_shape(70000, "float64", 128, 256) == (8, 4)
    assert mm.launch_shape(70000, "float64", 512, 256, 1) == (1, 4)


@pytest.mark.parametrize("cus", [256, 304])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_wave_plan_crosses_map_boundaries_in_tests_2_and_3(dtype, cus):
    # test 2: the genome at 1 Mb with the default waves per CU
    lay = mm.joint_layout(mm.GENOME_1MB, dtype)
    wpc, wpb = mm.launch_shape(lay["n_units"], dtype, lay["vw"], cus)
    plan = mm.wave_plan(lay["n_units"], lay["units_per_tile"], lay["tile_map"], cus, wpc, wpb)
    assert mm.crossing(plan)[0] >= 1
    # test 3: one wave per CU over 311 single-tile maps
    lay = mm.joint_layout(mm.THROUGH, dtype)
    assert lay["vw"] == 512 and lay["n_blocks"] == len(mm.THROUGH)
    assert lay["units_per_tile"] == (128 if dtype == "float32" else 256)
    wpc, wpb = mm.launch_shape(lay["n_units"], dtype, lay["vw"], cus, 1)
    plan = mm.wave_plan(lay["n_units"], lay["units_per_tile"], lay["tile_map"], cus, wpc, wpb)
    two, most, live = mm.crossing(plan)
    assert most >= 3 and 4 * two >= len(plan) and live == len(plan)


def test_history_batch_overflows_where_the_test_says():
    nm = len(mm.HISTORY)
    assert nm == 23
    most = mm.HIST_CAP // nm
    assert most * nm <= mm.HIST_CAP < (most + 1) * nm and most == 45590
