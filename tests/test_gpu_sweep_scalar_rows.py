"""GPU: the fp32 unit body reads a unit's twelve row coordinates from six scalar register pairs,
each subtract picking its half of a pair, and loads the next unit's over them row by row while it
runs (bb_solver_kernels.h: XRowS32, row_minus, xrow_refresh); the window's loads take a scalar
base and the lane's byte offset (WinBase32).  What can go wrong is a subtract that reads the wrong
half of a pair, a row that still holds (or already holds) another unit's coordinates, and a window
that points at another unit -- at the places where the body is entered by another path: a wave's
first unit, a strip change, a change of format, the wave's last unit.

So the start is one whose x, y and z differ by orders of magnitude in every bin and from bin to
bin (x = i, y = 1000 + 3 i, z = -7 i, plus seeded noise): a wrong half or a stale row shows in
the first digit of the gradient.  What must hold, as in tests/test_gpu_pack24_maskfree.py:

  - the exchange buffer of one grad(), the coordinates and the stress history are the SAME BITS with
    the stream (BB_PACK24=1: the packed and the raw body of stream24_grad_kernel) and without it
    (BB_PACK24=0: stress_grad_kernel);
  - gradient and stress agree with a float64 reference over the stored cells within SPEC 4's
    fp32 1e-5.

Every case runs at 1, 4 and 8 waves per CU (workgroups of 4 and of 8 waves), and shows from the
numpy model of the stream and of the wave chunks, evaluated for this device's CU count, that the
place it is about exists at the wave count that can hold it (long chunks: one wave per CU; chunks
of one unit: 8).  BB_ROW_OWNER_MAX=0 keeps these maps on the unit sweep; a case takes a fraction
of a second."""
import functools

import numpy
import pytest

from blueberry_amd.solver import HipEngine
from tests import _pack24_model as pm
from tests import _spectral_model as sm
from tests._pack24_model import RPU, UPT, VW
from tests.test_gpu_pack24 import _compare, _cu_count, _env, _same, _uniform_map
from tests.test_gpu_pack24_paths import TOL, _grad_error

pytestmark = pytest.mark.gpu

N1 = 4 * VW                                          # 10 tiles, 1,280 units
U1 = 10 * UPT
N2 = 1300                                            # 6 tiles, 768 units, the last strip ragged
U2 = 6 * UPT
WPC = [1, 4, 8]
STEPS = (2,)


def _start(n, seed=5):
    """Components that differ by orders of magnitude per bin and per component, exact in float32
    (the reference then starts from the coordinates the device holds)."""
    i = numpy.arange(n, dtype=numpy.float64)
    x = numpy.stack([i, 1000.0 + 3.0 * i, -7.0 * i], axis=1)
    x += numpy.random.default_rng(seed).normal(0.0, 0.25, (n, 3))
    return x.astype(numpy.float32).astype(numpy.float64)


@functools.lru_cache(maxsize=None)
def _map(n, seed=0):
    w = _uniform_map(n, seed=seed)
    w.setflags(write=False)
    return w


def _unit_cell(u, n, row=1, col=37):
    I, J = pm.dense_tiles(n)
    t, sub = divmod(u, UPT)
    return int(I[t]) * VW + sub * RPU + row, int(J[t]) * VW + col


def _zero_cell(w, u, n=N1):
    i, j = _unit_cell(u, n)
    w[i, j] = w[j, i] = 0.0


def _zero_unit(w, u, n=N1):
    i, j = _unit_cell(u, n, 0, 0)
    w[i:i + RPU, j:j + VW] = 0.0
    w[j:j + VW, i:i + RPU] = 0.0


def _chunks(n_units, wpc):
    cus = _cu_count()
    return pm.chunks(n_units, cus, wpc, pm.waves_per_block(n_units, cus, wpc)), cus


def _long_chunk(n_units, need, n=N1):
    """A chunk of one wave per CU with at least `need` units inside one off-diagonal tile, away
    from the tile's ends."""
    ch, cus = _chunks(n_units, 1)
    I, J = pm.dense_tiles(n)
    off = numpy.repeat(I < J, UPT)
    a, b = next(((a, b) for a, b in ch if b - a >= need and off[a:b].all() and a // UPT == (b - 1) // UPT
                 and a % UPT != 0 and b % UPT != 0), (0, 0))
    assert b - a >= need, "no chunk of %d units inside an off-diagonal tile (%d CUs)" % (need, cus)
    return a, b


def _stress_grad_q(w, n, X, q):
    """SPEC 2.3.1 in float64 over the stored cells (each pair once): S = sum delta^-q (d - delta)^2,
    d = sqrt(|x_i - x_j|^2 + 1e-30); tests/_pack24_model.stress_grad with the weight."""
    I, J = pm.dense_tiles(n)
    Xp = numpy.zeros((-(-n // VW) * VW, 3))
    Xp[:n] = X
    g = numpy.zeros_like(Xp)
    S = 0.0
    for t in range(I.size):
        delta = pm.stored_tile(w, n, int(I[t]), int(J[t])).astype(numpy.float64)
        r0, c0 = int(I[t]) * VW, int(J[t]) * VW
        diff = Xp[r0:r0 + VW, None, :] - Xp[None, c0:c0 + VW, :]
        d = numpy.sqrt((diff * diff).sum(-1) + pm.EPS2)
        on = delta > 0
        wq = numpy.where(on, numpy.where(on, delta, 1.0) ** (-float(q)), 0.0)
        res = numpy.where(on, d - delta, 0.0)
        S += float((wq * res * res).sum())
        f = (2.0 * wq * res / d)[:, :, None] * diff
        g[r0:r0 + VW] += f.sum(1)
        g[c0:c0 + VW] -= f.sum(0)
    return S, g[:n]


def _case(monkeypatch, w, n, n_units, x0, wpc, min_run, what):
    """The case with and without the stream (equal bits: _compare), the stream against its model,
    gradient and stress against the float64 reference.  Returns the packed mask."""
    on = _compare(monkeypatch, n, lambda e: e.set_wish_dense(w, "wish", 1.0), x0,
                  {"BB_PACK24_MIN_RUN": min_run, "BB_WAVES_PER_CU": wpc}, steps=STEPS)
    want, packed, _ = pm.model(w, n, 0, n_units, min_run)
    assert on["info"] == want
    S_ref, g_ref = pm.stress_grad(w, n, x0)
    err_g, err_s = _grad_error(on["grad"], g_ref, S_ref, n)
    print("%s, %d waves per CU: %d packed / %d raw units, %d format switches; gradient %.2e; stress %.2e"
          % (what, wpc, want["packed_units"], want["raw_units"], want["format_switches"], err_g, err_s))
    assert err_g < TOL and err_s < TOL, (err_g, err_s)
    return packed


# ---- 1, 2. a chunk that starts mid-strip; a strip change inside a chunk ------------------------------------
@pytest.mark.parametrize("wpc", WPC)
def test_chunk_starts_mid_strip_and_strip_change_inside_a_chunk(monkeypatch, wpc):
    """The map of tests/test_gpu_pack24.py: raw diagonal tiles, packed ones off the diagonal.  At
    every wave count most waves begin inside a strip and inside a tile, in a packed run and in a
    raw one: the prologue loads rows that are not a strip's first.  At one wave per CU the chunks
    are long enough for the strip changes to lie inside a chunk, with packed units on both sides
    and with a change of format at the change."""
    w, x0 = _map(N1), _start(N1)
    _, packed, _ = pm.model(w, N1, 0, U1, 1)
    strips = pm.strip_of_unit(N1)
    ch, cus = _chunks(U1, wpc)
    mid = [a for a, b in ch if a < b and a % UPT != 0 and strips[a] == strips[a - 1]]
    assert any(packed[a] for a in mid) and any(not packed[a] for a in mid), "%d CUs" % cus
    if wpc == 1:
        cross = pm.crossings(ch, strips, packed)
        assert cross["packed"] or cross["packed_raw"] or cross["raw_packed"] or cross["raw"], \
            "no strip change inside a chunk (%d CUs)" % cus
        assert len({u for a, b in ch for u in range(a + 1, b) if strips[u] != strips[u - 1]}) >= 2
    _case(monkeypatch, w, N1, U1, x0, wpc, 1, "mid-strip starts, strip changes")


# ---- 3. raw -> packed -> raw inside a chunk -------------------------------------------------------------------
@pytest.mark.parametrize("wpc", WPC)
def test_raw_packed_raw_inside_a_chunk(monkeypatch, wpc):
    """packed, RAW, packed, RAW, packed in the five units of one chunk of one wave per CU (a cell
    without a constraint makes a unit raw): each body hands the other a unit whose rows it
    fetched itself, twice in each direction."""
    a, b = _long_chunk(U1, 5)
    w, x0 = _map(N1).copy(), _start(N1)
    _zero_cell(w, a + 1)
    _zero_cell(w, a + 3)
    _, packed, table = pm.model(w, N1, 0, U1, 1)
    assert list(packed[a:a + 5]) == [True, False, True, False, True] and (table["base"][[a, a + 2, a + 4]] != 0).all()
    got = _case(monkeypatch, w, N1, U1, x0, wpc, 1, "raw, packed, raw at units %d..%d of chunk [%d, %d)" % (a + 1, a + 3, a, b))
    assert numpy.array_equal(got, packed)


# ---- 4. an all-zero packed unit -----------------------------------------------------------------------------------
@pytest.mark.parametrize("wpc", WPC)
def test_all_zero_packed_unit(monkeypatch, wpc):
    """A unit without any constraint between packed units of one chunk: packed with base 0, a run of
    one unit in the raw body, entered with window registers 6 and 7 set and left with the rows of
    the packed unit behind it."""
    a, b = _long_chunk(U1, 5)
    w, x0 = _map(N1).copy(), _start(N1)
    z = a + 2
    _zero_unit(w, z)
    _, packed, table = pm.model(w, N1, 0, U1, 1)
    zero = packed & (table["base"] == 0)
    assert zero[z] and zero.sum() == 1 and (packed[a:b] & ~zero[a:b]).sum() == b - a - 1
    _case(monkeypatch, w, N1, U1, x0, wpc, 1, "all-zero unit %d of chunk [%d, %d)" % (z, a, b))


# ---- 5. chunks of one unit ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("wpc", WPC)
def test_chunk_of_one_unit_ragged_size(monkeypatch, wpc):
    """N = 1,300 (768 units, padding rows and all-padding units in the last strip).  With 8 waves
    per CU a wave's chunk is one unit wherever the device has 96 CUs or more: the prologue's unit is
    the wave's last, and the rows its body fetches are, by the clamped descriptor, its own."""
    w, x0 = _map(N2, 1), _start(N2)
    ch, cus = _chunks(U2, wpc)
    if wpc == 8:
        assert all(b - a == 1 for a, b in ch if a < b) and len(ch) >= U2, "%d CUs" % cus
    _case(monkeypatch, w, N2, U2, x0, wpc, 1, "N = 1,300, chunks of up to %d" % max(b - a for a, b in ch))


# ---- 6. the weighted sweeps and the matvec ------------------------------------------------------------------
def _twin_engines(monkeypatch, wpc, n, w, run):
    """run(engine) with the stream and without it; the two results, equal bits asserted."""
    out = []
    for on in (1, 0):
        _env(monkeypatch, BB_PACK24=on, BB_PACK24_MIN_RUN=1, BB_WAVES_PER_CU=wpc)
        eng = HipEngine(n, "float32")
        try:
            eng.set_wish_dense(w, "wish", 1.0)
            assert (eng.stream_info()["packed_units"] > 0) == bool(on)
            out.append(run(eng))
        finally:
            eng.close()
    assert sorted(out[0]) == sorted(out[1])
    for key in out[0]:
        assert _same(out[0][key], out[1][key]), key
    return out[0]


@pytest.mark.parametrize("wpc", WPC)
@pytest.mark.parametrize("q", [1, 2])
def test_weighted_sweeps(monkeypatch, q, wpc):
    """kOpStressW1 and kOpStressW2 (SPEC 2.3.1) go through the same subtracts in stress_grad_kernel:
    one gradient and two steps on the map of case 3, against the weighted float64 reference."""
    a, _ = _long_chunk(U1, 5)
    w, x0 = _map(N1).copy(), _start(N1)
    _zero_cell(w, a + 1)
    _zero_cell(w, a + 3)

    def run(eng):
        eng.set_weight_power(q)
        eng.set_coords(x0)
        eng.grad()
        eng.sync()
        out = {"grad": eng.read_exchange()}
        eng.set_coords(x0)
        eng.iterate(2, 1.0 / (2.0 * N1))
        assert eng.iteration_path() == ("units", 0)
        out["X"], out["hist"] = eng.get_coords(), eng.stress_history()
        return out

    got = _twin_engines(monkeypatch, wpc, N1, w, run)
    S_ref, g_ref = _stress_grad_q(w, N1, x0, q)
    err_g, err_s = _grad_error(got["grad"], g_ref, S_ref, N1)
    err_h = float(abs(got["hist"][0] - S_ref) / S_ref)
    print("q = %d, %d waves per CU: gradient %.2e; stress %.2e; first history entry %.2e" % (q, wpc, err_g, err_s, err_h))
    assert err_g < TOL and err_s < TOL and err_h < TOL, (err_g, err_s, err_h)


@pytest.mark.parametrize("wpc", WPC)
def test_matvec(monkeypatch, wpc):
    """kOpMatvec2 reads a unit's row values from the same scalar pairs: (D o D) v for v = the start,
    whose components tell the halves apart, against the float64 product."""
    w, v = _map(N1), _start(N1)
    got = _twin_engines(monkeypatch, wpc, N1, w, lambda eng: {"y": eng.matvec_sq(v)})["y"]
    want = sm.matvec_sq_ref(w, v)
    err = float(numpy.abs(got - want).max() / numpy.abs(want).max())
    print("matvec, %d waves per CU: %.2e" % (wpc, err))
    assert got.shape == (N1, 3) and err < TOL, err
