"""GPU: the 24-bit stream of the fp32 stress sweep (docs/SPEC.md 3.7).  The sweep may read a copy
of its units in which runs of units whose 2,048 stored words span less than 2^24 as uint32 are
held as 6 KiB of offset codes.  What must hold:

  - a fit, a gradient and a stress history are the SAME BITS with the stream (BB_PACK24=1) and
    without it (BB_PACK24=0): there is no tolerance anywhere in this file;
  - which units are held packed follows the rule, as the numpy model of it says
    (tests/_pack24_model.py: packed units, raw units, stream bytes, format switches of
    `HipEngine.stream_info`).

Every map is small enough that a case takes a second or two; BB_ROW_OWNER_MAX=0 keeps the small
ones on the unit sweep."""
import numpy
import pytest

from blueberry_amd.solver import HipEngine
from tests import _oracle
from tests._pack24_model import RPU, SPAN, UPT, VW, model
from tests._pack24_model import uniform_map as _uniform_map
from tests._util import bits as _bits
from tests._util import cu_count as _cu_count

pytestmark = pytest.mark.gpu


def _same(a, b):
    """Equal under numpy.array_equal, bit pattern for bit pattern (a NaN equals itself)."""
    return numpy.array_equal(_bits(a), _bits(b))


def _env(monkeypatch, **env):
    for k in ("BB_PACK24", "BB_PACK24_MIN_RUN", "BB_WAVES_PER_CU", "BB_PAIR"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("BB_ROW_OWNER_MAX", "0")
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))


def _cell_of_unit(u, row=1, col=37):
    """A cell (i, j) of local unit u of a one-rank dense layout (strip-major: tile t = J (J + 1) / 2
    + I holds units t * 128 ..), off the diagonal tiles."""
    t, sub = divmod(u, UPT)
    J = int((numpy.sqrt(8.0 * t + 1.0) - 1.0) / 2.0)
    while J * (J + 1) // 2 > t:
        J -= 1
    while (J + 1) * (J + 2) // 2 <= t:
        J += 1
    I = t - J * (J + 1) // 2
    assert I < J, "a unit of a diagonal tile"
    return I * VW + sub * RPU + row, J * VW + col


def _run(n, set_wish, x0, steps=(7, 8), rank=0, world=1):
    """Everything a case compares: coordinates and stress history of `steps` steps at momentum 0
    and 0.5 (world 1: iterate; else grad + apply), one gradient, and the stream's description."""
    lr = 1.0 / (2.0 * n)
    out = {}
    eng = HipEngine(n, "float32", rank=rank, world=world)
    try:
        set_wish(eng)
        out["info"] = eng.stream_info()
        out["layout"] = eng.layout()
        eng.set_coords(x0)
        eng.grad()
        eng.sync()
        out["grad"] = eng.read_exchange()
    finally:
        eng.close()
    for mu in (0.0, 0.5):
        for k in steps:
            eng = HipEngine(n, "float32", rank=rank, world=world)
            try:
                set_wish(eng)
                eng.set_coords(x0)
                eng.set_momentum(mu)
                if world == 1:
                    eng.iterate(k, lr)
                    assert eng.iteration_path() == ("units", 0)
                else:
                    for _ in range(k):
                        eng.grad()
                        eng.apply(lr)
                out[(mu, k)] = (eng.get_coords(), eng.stress_history())
                assert out[(mu, k)][1].shape == (k,)
            finally:
                eng.close()
    return out


def _compare(monkeypatch, n, set_wish, x0, env, **kw):
    """The case with the stream and without it: equal bits.  Returns the run with the stream."""
    _env(monkeypatch, BB_PACK24=1, **env)
    on = _run(n, set_wish, x0, **kw)
    _env(monkeypatch, BB_PACK24=0, **env)
    off = _run(n, set_wish, x0, **kw)
    assert off["info"]["packed_units"] == 0 and off["info"]["stream_bytes"] == 0
    assert off["info"]["raw_units"] == off["layout"]["u_end"] - off["layout"]["u_begin"]
    assert numpy.count_nonzero(off["grad"]) > 0
    assert _same(on["grad"], off["grad"])
    for key in on:
        if isinstance(key, tuple):
            assert _same(on[key][0], off[key][0]), key
            assert _same(on[key][1], off[key][1]), key
    return on


def _check_model(on, w, n, min_run):
    want, packed, _ = model(w, n, on["layout"]["u_begin"], on["layout"]["u_end"], min_run)
    assert on["info"] == want
    return packed


N1 = 4 * VW                                          # 10 tiles, 1,280 units


@pytest.fixture(scope="module")
def map1():
    return _uniform_map(N1), _oracle.noisy_init(_oracle.random_walk(N1))


@pytest.mark.parametrize("wpc", [4, 8])
def test_diagonal_tiles_raw_all_others_packed(monkeypatch, map1, wpc):
    """Case 1: [1, 1.9] lies in one binade, so every unit off the diagonal tiles packs; a unit of
    a diagonal tile holds the 0 of its diagonal beside distances and stays raw.  Both workgroup
    forms (4 and 8 waves)."""
    w, x0 = map1
    on = _compare(monkeypatch, N1, lambda e: e.set_wish_dense(w, "wish", 1.0), x0,
                  {"BB_PACK24_MIN_RUN": 1, "BB_WAVES_PER_CU": wpc})
    packed = _check_model(on, w, N1, 1)
    assert on["info"]["packed_units"] == 6 * UPT and on["info"]["raw_units"] == 4 * UPT
    assert not packed[:UPT].any() and packed[UPT:2 * UPT].all()


def test_ragged_size(monkeypatch):
    """Case 2: N = 1,300.  Units that mix padding zeros with distances come out raw (every unit of
    the last strip with a real row), all-zero padding units packed with base 0."""
    n = 1300
    w = _uniform_map(n, seed=1)
    x0 = _oracle.noisy_init(_oracle.random_walk(n))
    on = _compare(monkeypatch, n, lambda e: e.set_wish_dense(w, "wish", 1.0), x0, {"BB_PACK24_MIN_RUN": 1})
    packed = _check_model(on, w, n, 1)
    first_pad = (n - 2 * VW + RPU - 1) // RPU        # first all-padding unit of tile (2, 2)
    assert not packed[3 * UPT:5 * UPT + first_pad].any()     # tiles (0,2), (1,2), real rows of (2,2)
    assert packed[5 * UPT + first_pad:].all() and packed[UPT:2 * UPT].all()


@pytest.mark.parametrize("min_run", [1, 3, 64])
def test_single_raw_units_inside_packed_runs(monkeypatch, map1, min_run):
    """Case 3: a 0 in one cell of chosen units of case 1's map, chosen from the chunks the solver
    cuts: with one wave per CU the 1,280 units go to `cus` waves (rounded up to a workgroup of 4),
    the first r of them one unit longer.  On 256 CUs a chunk is 5 units and the raw units are 130
    (first of wave 26's), 133, 134 (last of it; 131 and 132 are a packable run of two between raw
    units), 139 (last of wave 27's) and 200 (first of wave 40's)."""
    cus = _cu_count()
    nw = min(-(-cus // 4) * 4, 10 * UPT)
    q, r = divmod(10 * UPT, nw)
    assert q >= 5, "chunks of %d units: too short for this case's raw units (%d CUs)" % (q, cus)
    start = lambda k: k * q + min(k, r)                # first unit of wave k's chunk
    k1 = next(k for k in range(nw) if start(k) > UPT)          # a chunk inside tile (0, 1)
    k3 = next(k for k in range(nw) if start(k) >= UPT + 70)    # a later one in the same tile
    raw = [start(k1), start(k1) + 3, start(k1 + 1) - 1, start(k1 + 2) - 1, start(k3)]
    assert raw[-1] < 2 * UPT and len(set(raw)) == 5
    if cus == 256:
        assert raw == [130, 133, 134, 139, 200]
    w, x0 = map1
    w = w.copy()
    for u in raw:
        i, j = _cell_of_unit(u)
        w[i, j] = w[j, i] = 0.0
    on = _compare(monkeypatch, N1, lambda e: e.set_wish_dense(w, "wish", 1.0), x0,
                  {"BB_PACK24_MIN_RUN": min_run, "BB_WAVES_PER_CU": 1})
    packed = _check_model(on, w, N1, min_run)
    assert not packed[raw].any()
    assert packed[3 * UPT:5 * UPT].all()
    assert packed[raw[0] + 1:raw[1]].all() == (min_run <= 2)
    assert packed[raw[3] + 1:raw[4]].all() == (min_run <= raw[4] - raw[3] - 1)


@pytest.mark.parametrize("top", [0x3f800000 + SPAN, 0x7f7fffff])
def test_boundary_of_the_packable_test(monkeypatch, top):
    """Case 4: words spanning exactly 2^24 - 1 pack, words spanning exactly 2^24 do not; from
    float32 bit patterns around 1.0 and below the largest finite value."""
    def f32(bits):
        return numpy.array(bits, dtype=numpy.uint32).view(numpy.float32).astype(numpy.float64)
    lo = top - SPAN                                   # the raw unit spans [lo, top]
    rng = numpy.random.default_rng(2)
    w = f32(rng.integers(lo + 1, lo + (SPAN >> 1), (N1, N1), dtype=numpy.uint32))
    w = numpy.triu(w, 1)
    w = w + w.T
    for u, (a, b) in ((133, (lo + 1, top)), (150, (lo, top))):     # span 2^24 - 1, span 2^24
        (i, j), (i2, j2) = _cell_of_unit(u, 0, 5), _cell_of_unit(u, 3, 500)
        w[i, j] = w[j, i] = f32(a)
        w[i2, j2] = w[j2, i2] = f32(b)
    x0 = _oracle.noisy_init(_oracle.random_walk(N1))
    on = _compare(monkeypatch, N1, lambda e: e.set_wish_dense(w, "wish", 1.0), x0, {"BB_PACK24_MIN_RUN": 1})
    packed = _check_model(on, w, N1, 1)
    assert packed[133] and not packed[150] and packed[149] and packed[151]


def test_natural_mix(monkeypatch):
    """Case 5: N = 17,000 from random-walk coordinates, 76,160 units in workgroups of 8 waves,
    the default run rule, 3 steps."""
    n = 17000
    xs = _oracle.random_walk(n)
    x0 = _oracle.noisy_init(xs)
    on = _compare(monkeypatch, n, lambda e: e.set_wish_from_coords(xs), x0, {}, steps=(3,))
    info = on["info"]
    assert info["packed_units"] + info["raw_units"] == 595 * UPT
    assert info["packed_units"] > info["raw_units"] > 0 and info["format_switches"] > 0


def test_second_rank_of_two(monkeypatch, map1):
    """Case 6: case 1 on rank 1 of 2, whose first unit is not the map's first."""
    w, x0 = map1
    on = _compare(monkeypatch, N1, lambda e: e.set_wish_dense(w, "wish", 1.0), x0,
                  {"BB_PACK24_MIN_RUN": 1}, rank=1, world=2)
    assert on["layout"]["u_begin"] > 0
    _check_model(on, w, N1, 1)
    assert on["info"]["packed_units"] > 0 and on["info"]["raw_units"] > 0


def test_zero_in_every_unit_means_no_stream(monkeypatch, map1):
    """Case 7: a 0 in column 3 of every strip puts one into every unit: nothing packs, and the
    solver reports no stream."""
    w, x0 = map1
    w = w.copy()
    w[:, 3::VW] = 0.0
    w[3::VW, :] = 0.0
    on = _compare(monkeypatch, N1, lambda e: e.set_wish_dense(w, "wish", 1.0), x0, {"BB_PACK24_MIN_RUN": 1})
    assert on["info"] == {"packed_units": 0, "raw_units": 10 * UPT, "stream_bytes": 0, "format_switches": 0}
    _check_model(on, w, N1, 1)
