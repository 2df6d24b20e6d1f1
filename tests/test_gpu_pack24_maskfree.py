"""GPU: the two bodies of the sweep over the 24-bit stream (docs/SPEC.md 3.7).  A packed unit whose
base is not 0 holds no zero and runs in a body WITHOUT the empty-pair mask; a packed unit with
base 0 is all zeros and runs in the raw body, alone in its run.  What must hold, as in
tests/test_gpu_pack24.py:

  - the exchange buffer of one grad(), the coordinates and the stress history are the SAME BITS with
    the stream (BB_PACK24=1) and without it (BB_PACK24=0), the sign of every zero included (the
    comparison is of uint64 views): there is no tolerance on that;
  - gradient and stress agree with the float64 reference over the stored cells
    (tests/_pack24_model.stress_grad) within SPEC 4's fp32 1e-5, as in tests/test_gpu_pack24_paths.py.

Every case shows from the numpy model of the stream and of the wave chunks, evaluated for this
device's CU count, that its units are what it says -- packed with base 0, packed with another
base, raw -- and lie where it says in a wave's chunk and beside a strip change.  A device on which
that cannot be had fails the case.  BB_ROW_OWNER_MAX=0 keeps these maps on the unit sweep; a case
takes a second or two."""
import numpy
import pytest

from tests import _oracle
from tests import _pack24_model as pm
from tests._pack24_model import RPU, UPT, VW
from tests.test_gpu_pack24 import _compare, _cu_count, _uniform_map
from tests.test_gpu_pack24_paths import TOL, _grad_error

pytestmark = pytest.mark.gpu

N1 = 4 * VW                                          # 10 tiles, 1,280 units
U1 = 10 * UPT
TILES1 = pm.dense_tiles(N1)


def _rows_cols(u, n=N1):
    """(first row, first column) of unit u of the dense layout."""
    I, J = pm.dense_tiles(n)
    t, sub = divmod(u, UPT)
    return int(I[t]) * VW + sub * RPU, int(J[t]) * VW


def _zero_unit(w, u, n=N1):
    """The unit's 4 rows x 512 columns (both triangles) without a constraint."""
    i, j = _rows_cols(u, n)
    w[i:i + RPU, j:j + VW] = 0.0
    w[j:j + VW, i:i + RPU] = 0.0


def _zero_cell(w, u, row=1, col=37, n=N1):
    i, j = _rows_cols(u, n)
    w[i + row, j + col] = w[j + col, i + row] = 0.0


def _off_diagonal(n=N1):
    """Per unit: it belongs to a tile off the diagonal (every cell of it is stored)."""
    I, J = pm.dense_tiles(n)
    return numpy.repeat(I < J, UPT)


def _chunks(n_units, wpc):
    cus = _cu_count()
    return pm.chunks(n_units, cus, wpc, pm.waves_per_block(n_units, cus, wpc)), cus


def _chunk_of(ch, u):
    return next((a, b) for a, b in ch if a <= u < b)


def _model(w, n, min_run=1):
    n_units = len(pm.dense_tiles(n)[0]) * UPT
    info, packed, table = pm.model(w, n, 0, n_units, min_run)
    zero = packed & (table["base"] == 0)              # the raw body, one unit per run
    free = packed & (table["base"] != 0)              # the body without the mask
    return info, packed, zero, free


def _against_reference(on, w, n, x0, what):
    S_ref, g_ref = pm.stress_grad(w, n, x0)
    err_g, err_s = _grad_error(on["grad"], g_ref, S_ref, n)
    print("%s: %d packed / %d raw units, %d format switches; gradient %.2e; stress %.2e"
          % (what, on["info"]["packed_units"], on["info"]["raw_units"], on["info"]["format_switches"],
             err_g, err_s))
    assert err_g < TOL and err_s < TOL, (err_g, err_s)


@pytest.fixture(scope="module")
def map1():
    return _uniform_map(N1), _oracle.noisy_init(_oracle.random_walk(N1))


# ---- 1. zero units between packed units -------------------------------------------------------------------
def _place_zero_units(ch, strips, off):
    """Where case 1 puts its zero units, from the chunks this device cuts: `first` opens a chunk,
    `last` closes one, `pair` are two consecutive units, `behind` is the first unit of a strip,
    `before` the last one of a strip.  The chunks are as long as the device leaves them (L units at
    the most): with L >= 2 `first`, `last` and `pair` each lie in a chunk of their own of at least
    min(L, 3) units of one off-diagonal tile, so that `first` is followed and `last` preceded by a
    unit of the same chunk, and the pair lies inside one chunk; `behind` and `before` are taken
    inside a chunk (the change is one the wave itself crosses) where any chunk holds a change."""
    L = max(b - a for a, b in ch)
    need = min(L, 3)
    whole = [(a, b) for a, b in ch if b - a >= need and off[a:b].all() and len(set(strips[a:b])) == 1
             and a % UPT != 0 and b % UPT != 0]
    assert len(whole) >= 5, "no five chunks of %d units inside off-diagonal tiles" % need
    first, last, pair = whole[1][0], whole[2][1] - 1, whole[4][0] + (1 if need == 3 else 0)
    changes = [u for u in range(1, len(strips)) if strips[u] != strips[u - 1]]
    inside = [u for u in changes if _chunk_of(ch, u)[0] < u]
    behind = (inside or changes)[0]
    before = ([u for u in inside if u != behind] or [u for u in changes if u != behind])[-1] - 1
    return {"first": first, "last": last, "pair": pair, "behind": behind, "before": before,
            "L": L, "inside": inside}


@pytest.mark.parametrize("wpc", [1, 4, 8])
def test_zero_units_between_packed_units(monkeypatch, map1, wpc):
    """Whole units without a constraint in a map whose other off-diagonal units pack with a base
    above 0: the first and the last unit of a wave's chunk, two in a row, the first unit behind a
    strip change and the last one before a strip change (that one closes a diagonal tile: raw
    units before it, a packed one behind it).  Workgroups of 4 waves (1 and 4 waves per CU) and of
    8; at one wave per CU the chunks are long enough (asserted) for every place to lie INSIDE a
    chunk, the strip changes included."""
    w, x0 = map1
    w = w.copy()
    strips = pm.strip_of_unit(N1)
    ch, cus = _chunks(U1, wpc)
    assert pm.waves_per_block(U1, cus, wpc) == (8 if wpc == 8 else 4)
    at = _place_zero_units(ch, strips, _off_diagonal())
    zeros = [at["first"], at["last"], at["pair"], at["pair"] + 1, at["behind"], at["before"]]
    assert len(set(zeros)) == 6
    for u in zeros:
        _zero_unit(w, u)
    _, packed, zero, free = _model(w, N1)
    assert zero[zeros].all() and zero.sum() == 6, "the chosen units: packed with base 0, and no others"
    assert _chunk_of(ch, at["first"])[0] == at["first"] and _chunk_of(ch, at["last"])[1] == at["last"] + 1
    assert strips[at["behind"]] != strips[at["behind"] - 1] and strips[at["before"]] != strips[at["before"] + 1]
    assert not packed[at["before"] - 1] and free[at["before"] + 1] and free[at["behind"] + 1]
    assert free[at["pair"] - 1] and free[at["pair"] + 2]
    if wpc == 1:
        assert at["L"] >= 3 and len(at["inside"]) >= 2, \
            "chunks of %d units, strip changes inside a chunk at %r (%d CUs)" % (at["L"], at["inside"], cus)
    if at["L"] >= 2:
        a, b = _chunk_of(ch, at["first"])
        assert b - a >= 2 and free[a + 1:b].all()
        a, b = _chunk_of(ch, at["last"])
        assert b - a >= 2 and free[a:b - 1].all()
        assert _chunk_of(ch, at["pair"]) == _chunk_of(ch, at["pair"] + 1)
    if len(at["inside"]) >= 2:
        a, b = _chunk_of(ch, at["behind"])
        assert a < at["behind"]
        a, b = _chunk_of(ch, at["before"])
        assert at["before"] + 1 < b
    on = _compare(monkeypatch, N1, lambda e: e.set_wish_dense(w, "wish", 1.0), x0,
                  {"BB_PACK24_MIN_RUN": 1, "BB_WAVES_PER_CU": wpc})
    assert on["info"] == pm.model(w, N1, 0, U1, 1)[0]
    _against_reference(on, w, N1, x0, "zero units %r, %d waves per CU, chunks of up to %d" % (zeros, wpc, at["L"]))


# ---- 2. a zero unit beside truly raw units ---------------------------------------------------------------
def test_zero_unit_between_raw_units(monkeypatch, map1):
    """packed, RAW (one cell without a constraint), ZERO, RAW, packed inside one wave's chunk: the
    raw run before the zero unit ends at it, the one behind it asks for its own loads 6 and 7."""
    w, x0 = map1
    w = w.copy()
    ch, cus = _chunks(U1, 1)
    off = _off_diagonal()
    a, b = next(((a, b) for a, b in ch if b - a >= 5 and off[a:b].all() and a > UPT), (0, 0))
    assert b - a >= 5, "no chunk of 5 units inside an off-diagonal tile (%d CUs)" % cus
    z = a + 2
    _zero_cell(w, z - 1)
    _zero_unit(w, z)
    _zero_cell(w, z + 1)
    _, packed, zero, free = _model(w, N1)
    assert zero[z] and zero.sum() == 1
    assert not packed[z - 1] and not packed[z + 1] and free[z - 2] and free[z + 2]
    on = _compare(monkeypatch, N1, lambda e: e.set_wish_dense(w, "wish", 1.0), x0,
                  {"BB_PACK24_MIN_RUN": 1, "BB_WAVES_PER_CU": 1})
    assert on["info"] == pm.model(w, N1, 0, U1, 1)[0]
    _against_reference(on, w, N1, x0, "raw, zero, raw at units %d..%d of chunk [%d, %d)" % (z - 1, z + 1, a, b))


# ---- 3. bins without any constraint ---------------------------------------------------------------------
def test_bins_without_any_constraint(monkeypatch, map1):
    """Bins 40..43 (one unit's rows) have no pair at all: their unit is all zero in every strip and
    their gradient is a sum of zeros, whose signs are the raw body's.  The start puts them below
    every other bin in x and above in y, so that their zero forces come with either sign."""
    w, x0 = map1
    w, x0 = w.copy(), x0.copy()
    rows = numpy.arange(40, 40 + RPU)
    w[rows, :] = 0.0
    w[:, rows] = 0.0
    x0[rows, 0] = x0[:, 0].min() - 1.0 - 0.25 * numpy.arange(RPU)
    x0[rows, 1] = x0[:, 1].max() + 1.0 + 0.25 * numpy.arange(RPU)
    units = [t * UPT + 10 for t in range(10) if TILES1[0][t] == 0]       # tiles (0, J), unit 10
    assert units == [10, UPT + 10, 3 * UPT + 10, 6 * UPT + 10]
    _, packed, zero, free = _model(w, N1)
    assert zero[units].all() and zero.sum() == 4
    for u in units[1:]:
        assert free[u - 1] and free[u + 1]
    ch, cus = _chunks(U1, 1)
    assert any(a < u < b - 1 for u in units[1:] for a, b in ch), "no such unit inside a chunk (%d CUs)" % cus
    on = _compare(monkeypatch, N1, lambda e: e.set_wish_dense(w, "wish", 1.0), x0,
                  {"BB_PACK24_MIN_RUN": 1, "BB_WAVES_PER_CU": 1})
    assert on["info"] == pm.model(w, N1, 0, U1, 1)[0]
    g = on["grad"][:3 * N1].reshape(N1, 3)
    assert not g[rows].any() and numpy.count_nonzero(g) > 0
    for key in on:
        if isinstance(key, tuple):                   # bins without a pair stay where they were
            assert numpy.array_equal(on[key][0][rows], x0[rows].astype(numpy.float32).astype(numpy.float64)), key
    _against_reference(on, w, N1, x0, "bins 40..43 without a pair")


# ---- 4. the floor ------------------------------------------------------------------------------------------
def test_smallest_distances_in_the_body_without_the_mask(monkeypatch, map1):
    """Tile (1, 3) holds float32 bit patterns from the smallest stored distance (the first float32
    at or above 1e-30) to 1.5e-30: packable with a base above 0, the smallest weight-1 distances
    the body without the mask can meet.  A cell of tile (0, 3) one bit pattern below the floor is
    flushed to 0 and makes its unit raw."""
    w, x0 = map1
    w = w.copy()
    f32 = lambda bits: numpy.asarray(bits, dtype=numpy.uint32).view(numpy.float32).astype(numpy.float64)
    lo = int(numpy.array(pm.WISH_FLOOR, dtype=numpy.float32).view(numpy.uint32))
    while f32(lo) < pm.WISH_FLOOR:
        lo += 1
    hi = int(numpy.array(1.5e-30, dtype=numpy.float32).view(numpy.uint32))
    assert f32(lo - 1) < pm.WISH_FLOOR <= f32(lo) and 0 < hi - lo < pm.SPAN and lo > pm.SPAN
    t13 = [t for t in range(10) if (TILES1[0][t], TILES1[1][t]) == (1, 3)][0]
    tile = f32(numpy.random.default_rng(4).integers(lo, hi + 1, (VW, VW), dtype=numpy.uint32))
    tile[0, 0], tile[VW - 1, VW - 1] = f32(lo), f32(hi)
    w[VW:2 * VW, 3 * VW:] = tile
    w[3 * VW:, VW:2 * VW] = tile.T
    below = 6 * UPT + 77                              # a unit of tile (0, 3)
    i, j = _rows_cols(below)
    w[i + 2, j + 300] = w[j + 300, i + 2] = f32(lo - 1)
    _, packed, zero, free = _model(w, N1)
    assert free[t13 * UPT:(t13 + 1) * UPT].all() and not zero.any()
    assert not packed[below] and free[below - 1] and free[below + 1]
    on = _compare(monkeypatch, N1, lambda e: e.set_wish_dense(w, "wish", 1.0), x0, {"BB_PACK24_MIN_RUN": 1})
    assert on["info"] == pm.model(w, N1, 0, U1, 1)[0]
    _against_reference(on, w, N1, x0, "distances of [1e-30, 1.5e-30] in tile (1, 3)")


# ---- 5. N = 1,300 --------------------------------------------------------------------------------------------
def test_ragged_size_zero_run_at_the_end_of_a_chunk(monkeypatch):
    """The ragged map of tests/test_gpu_pack24.py, 1 and 2 steps, momentum 0 and 0.5, runs of 3 or
    more: the all-padding units of tile (2, 2) are one packed run of zero units, which a wave
    meets behind raw units and as the last units of its chunk."""
    n = 1300
    w = _uniform_map(n, seed=1)
    x0 = _oracle.noisy_init(_oracle.random_walk(n))
    n_units = 6 * UPT
    first_pad = 5 * UPT + (n - 2 * VW + RPU - 1) // RPU
    _, packed, zero, free = _model(w, n, 3)
    assert zero[first_pad:].all() and zero.sum() == n_units - first_pad and not packed[3 * UPT:first_pad].any()
    assert free[UPT:2 * UPT].all()
    ch, cus = _chunks(n_units, 1)
    assert any(b - max(a, first_pad) >= 2 for a, b in ch if b > first_pad), \
        "no chunk ends in two zero units (%d CUs)" % cus
    on = _compare(monkeypatch, n, lambda e: e.set_wish_dense(w, "wish", 1.0), x0,
                  {"BB_PACK24_MIN_RUN": 3, "BB_WAVES_PER_CU": 1}, steps=(1, 2))
    assert on["info"] == pm.model(w, n, 0, n_units, 3)[0]
    _against_reference(on, w, n, x0, "N = 1,300, %d zero units from %d on" % (n_units - first_pad, first_pad))
