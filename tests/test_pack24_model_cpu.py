"""CPU: tests/_pack24_model.py, the numpy restatement of the 24-bit stream's rules (docs/SPEC.md
3.7) that the GPU tests hold `stream_info` against: the numbers the dense cases assert, the span
boundary, the run rule, the table, the wave chunk rule and the strip changes inside a chunk, and
the float64 reference against the oracle."""
import numpy
import pytest

from tests import _oracle
from tests import _pack24_model as pm
from tests._pack24_model import RPU, SPAN, UPT, VW
from tests._pack24_model import uniform_map as _uniform_map


def test_dense_2048_diagonal_tiles_raw_all_others_packed():
    n = 4 * VW
    info, packed, table = pm.model(_uniform_map(n), n, 0, 10 * UPT, 1)
    assert info == {"packed_units": 6 * UPT, "raw_units": 4 * UPT,
                    "stream_bytes": 1024 * (6 * 6 * UPT + 8 * 4 * UPT), "format_switches": 6}
    I, J = pm.dense_tiles(n)
    for t in range(10):
        assert packed[t * UPT:(t + 1) * UPT].all() == (I[t] != J[t])
        assert packed[t * UPT:(t + 1) * UPT].any() == (I[t] != J[t])
    assert numpy.array_equal(I, _oracle.dense_tiles(n)[0]) and numpy.array_equal(J, _oracle.dense_tiles(n)[1])
    # a base lies in [1, 2)'s binade when packed, and is 0 otherwise
    assert (table["base"][~packed] == 0).all()
    assert ((table["base"][packed] >= 0x3f800000) & (table["base"][packed] < 0x40000000)).all()


def test_ragged_1300_split():
    n = 1300
    info, packed, _ = pm.model(_uniform_map(n, seed=1), n, 0, 6 * UPT, 1)
    first_pad = (n - 2 * VW + RPU - 1) // RPU
    assert first_pad == 69
    assert not packed[:UPT].any() and packed[UPT:2 * UPT].all() and not packed[2 * UPT:3 * UPT].any()
    assert not packed[3 * UPT:5 * UPT + first_pad].any()
    assert packed[5 * UPT + first_pad:].all()
    assert info["packed_units"] == UPT + (UPT - first_pad)
    assert info["raw_units"] == 6 * UPT - info["packed_units"]
    assert info["format_switches"] == 3


def test_unit_range_of_a_rank():
    n = 4 * VW
    w = _uniform_map(n)
    whole = pm.model(w, n, 0, 10 * UPT, 1)[1]
    assert pm.rank_range(10 * UPT, 1, 2) == (640, 1280) and pm.rank_range(1280, 2, 3) == (853, 1280)
    for rank, world in ((1, 2), (2, 3), (0, 3)):
        a, b = pm.rank_range(10 * UPT, rank, world)
        info, packed, table = pm.model(w, n, a, b, 1)
        assert numpy.array_equal(packed, whole[a:b]) and table["offset_kib"][0] == 0
        assert info["packed_units"] + info["raw_units"] == b - a


def _f32(bits):
    return numpy.array(bits, dtype=numpy.uint32).view(numpy.float32).astype(numpy.float64)


@pytest.mark.parametrize("top", [0x3f800000 + SPAN, 0x7f7fffff])
def test_span_boundary(top):
    """Words spanning 2^24 - 1 pack, words spanning 2^24 do not."""
    n = 2 * VW
    lo = top - SPAN
    w = numpy.full((n, n), float(_f32(lo + 5)))
    numpy.fill_diagonal(w, 0.0)
    for unit, (a, b) in ((3, (lo + 1, top)), (9, (lo, top))):
        i = unit * RPU
        w[i, VW + 5] = w[VW + 5, i] = _f32(a)
        w[i + 3, VW + 500] = w[VW + 500, i + 3] = _f32(b)
    _, packed, table = pm.model(w, n, 0, 3 * UPT, 1)
    assert packed[UPT + 3] and not packed[UPT + 9] and packed[UPT + 8] and packed[UPT + 10]
    assert table["base"][UPT + 3] == lo + 1 and table["base"][UPT + 9] == 0
    lo_w, hi_w = pm.unit_spans(w, n)
    assert hi_w[UPT + 3] - lo_w[UPT + 3] == SPAN - 1 and hi_w[UPT + 9] - lo_w[UPT + 9] == SPAN


def test_what_is_no_constraint_is_stored_as_zero():
    n = VW + 3
    w = _uniform_map(n)
    for k, v in enumerate((numpy.nan, numpy.inf, -1.0, 1e-31, 1e39)):
        w[k, VW + 1] = w[VW + 1, k] = v
    tile = pm.stored_tile(w, n, 0, 1)
    assert not tile[:5, 1].any() and tile[5, 1] == numpy.float32(w[5, VW + 1])
    assert not tile[:, 3:].any() and tile[:, :3].all(0).tolist() == [True, False, True]
    diag = pm.stored_tile(w, n, 0, 0)
    assert not numpy.tril(diag).any() and numpy.triu(diag, 1)[0, 1:].all()


@pytest.mark.parametrize("R", [2, 3, 64])
def test_run_rule_at_its_edges(R):
    """Runs of R - 1, R and R + 1 packable units between raw ones: the first stays raw."""
    packable = []
    for length in (R - 1, R, R + 1):
        packable += [False] + [True] * length
    packable += [False]
    packed = pm.run_rule(packable, R)
    want = [False] * R + [False] + [True] * R + [False] + [True] * (R + 1) + [False]
    assert packed.tolist() == want
    assert pm.run_rule(packable, 1).tolist() == packable
    assert not pm.run_rule(packable, R + 2).any()


def test_table_offsets_are_cumulative_and_bytes_add_up():
    rng = numpy.random.default_rng(5)
    packed = rng.random(777) < 0.6
    base = rng.integers(1, 1 << 30, 777)
    info, table = pm.describe(packed, base)
    p, r = int(packed.sum()), int((~packed).sum())
    assert info["packed_units"] == p and info["raw_units"] == r
    assert info["stream_bytes"] == 1024 * (6 * p + 8 * r)
    off = table["offset_kib"]
    assert off[0] == 0
    assert numpy.array_equal(numpy.diff(off), numpy.where(packed[:-1], 6, 8))
    assert off[-1] + (6 if packed[-1] else 8) == info["stream_bytes"] // 1024
    assert numpy.array_equal(table["base"], numpy.where(packed, base, 0))
    assert info["format_switches"] == sum(1 for a, b in zip(packed[1:], packed[:-1]) if a != b)
    none, table0 = pm.describe(numpy.zeros(5, dtype=bool), numpy.arange(5))
    assert none == {"packed_units": 0, "raw_units": 5, "stream_bytes": 0, "format_switches": 0}
    assert table0["offset_kib"].tolist() == [0, 8, 16, 24, 32]


@pytest.mark.parametrize("wpc", [1, 4, 8])
@pytest.mark.parametrize("cus", [64, 256, 304])
@pytest.mark.parametrize("n_local", [1, 7, 640, 1280, 76160])
def test_chunk_rule(n_local, cus, wpc):
    wpb = pm.waves_per_block(n_local, cus, wpc)
    assert wpb == (8 if wpc == 8 and n_local >= 8 else 4)
    ch = pm.chunks(n_local, cus, wpc, wpb)
    assert len(ch) % wpb == 0 and len(ch) - wpb < max(1, min(cus * wpc, n_local)) <= len(ch)
    sizes = [b - a for a, b in ch]
    assert sum(sizes) == n_local and max(sizes) - min(sizes) <= 1
    assert sizes == sorted(sizes, reverse=True)
    assert ch[0][0] == 0 and all(ch[k][1] == ch[k + 1][0] for k in range(len(ch) - 1))


def test_chunks_on_256_cus():
    assert pm.chunks(1280, 256, 1, 4)[26] == (130, 135)
    ch = pm.chunks(640, 256, 1, 4)
    assert ch[:3] == [(0, 3), (3, 6), (6, 9)] and ch[128] == (384, 386) and ch[-1] == (638, 640)


def test_crossings_finds_a_planted_case_of_each_kind():
    strips = numpy.repeat([1, 3, 5, 7], 6)
    ch = [(0, 5), (5, 8), (8, 11), (11, 14), (14, 19), (19, 24)]
    # changes at units 6 (wave 1), 12 (wave 3), 18 (wave 4)
    packed = numpy.ones(24, dtype=bool)
    assert pm.crossings(ch, strips, packed) == {"packed": [1, 3, 4], "packed_raw": [], "raw_packed": [], "raw": []}
    packed[5] = False                                      # raw before the change at 6
    packed[12] = False                                     # raw behind the change at 12
    packed[17:19] = False                                  # a raw pair around the change at 18
    assert pm.crossings(ch, strips, packed) == {"packed": [], "packed_raw": [3], "raw_packed": [1], "raw": [4]}
    # a change that falls between two chunks is none
    assert pm.crossings([(0, 6), (6, 12)], strips[:12], packed[:12]) == \
        {"packed": [], "packed_raw": [], "raw_packed": [], "raw": []}
    assert pm.strip_of_unit(2 * VW).tolist() == [0] * UPT + [1] * (2 * UPT)
    tiles = (numpy.array([0, 2]), numpy.array([1, 3]))
    assert pm.strip_of_unit(4 * VW, tiles, 100, 130).tolist() == [1] * 28 + [3] * 2


def test_reference_against_the_oracle():
    """The float64 reference of a tile list = the oracle's sum over the same units, and its steps
    on a dense map = the oracle's."""
    n = 2 * VW + 40
    w = _uniform_map(n, seed=3)
    w[7, 900] = w[900, 7] = 0.0
    xs = _oracle.random_walk(n)
    x0 = _oracle.noisy_init(xs)
    o = _oracle.load()
    tiles = (numpy.array([0, 1, 0], dtype=numpy.int32), numpy.array([1, 1, 2], dtype=numpy.int32))
    for a, b in ((0, 3 * UPT), (70, 300), (128, 129)):
        s_ref, g_ref = o.stress_grad_units(w, x0, tiles[0], tiles[1], UPT, VW, a, b)
        s, g = pm.stress_grad(w, n, x0, tiles, a, b)
        assert abs(s / s_ref - 1) < 1e-12
        assert numpy.abs(g - g_ref).max() < 1e-12 * numpy.abs(g_ref).max()
    lr = 1.0 / (2.0 * n)
    scale = numpy.random.default_rng(4).uniform(0.5, 1.0, n)
    for mu, sc in ((0.0, None), (0.5, scale)):
        X_ref, h_ref = o.solve_weighted(w, x0, 3, lr, 0, mu=mu, bin_scale=sc)
        X, h = pm.run(w, n, x0, 3, lr, mu=mu, bin_scale=sc)
        assert numpy.abs(h / h_ref - 1).max() < 1e-12
        assert numpy.abs(X - X_ref).max() < 1e-12 * numpy.abs(X_ref).max()
    I, J = pm.dense_tiles(5 * VW)
    mI, mJ = pm.map_tiles((I, J), [0, 1024, 2560], 1)
    assert list(zip(mI.tolist(), mJ.tolist())) == [(2, 2), (2, 3), (3, 3), (2, 4), (3, 4), (4, 4)]
