"""The sequences of calls in which a handle frees, re-makes or hands over what it owns: the
solver's tables and buffers (bb::DevBuf members), its events (bb::Event), the triples and a
group that is refused.  Each sequence must leave the handle -- and the device -- computing
exactly what a fresh handle computes from the same inputs: the library promises the same bits
on every run (test_gpu_parity.py::test_solver_bitwise_reproducible), so every comparison is
numpy.array_equal, without a tolerance.

Sizes: fp32 at N = 1,100 (three blocks of 512, the last one partial) and fp64 at N = 300 (the
narrow layout: blocks of 128), each on the row-owner path and on the unit sweep
(BB_ROW_OWNER_MAX=0) unless a case says why not."""
import ctypes
import os
import subprocess
import sys

import numpy
import pytest

from blueberry_amd import _lib
from blueberry_amd.solver import DeviceTriples, HipEngine, layout_info
from tests import _oracle
from tests._util import solver_path                   # noqa: F401 -- a fixture

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

K = 5
SIZES = [("float32", 1100), ("float64", 300)]
# diagonal blocks and one off-diagonal tile inside the second map: no tile joins two maps
TILES = (numpy.array([0, 1, 1, 2], dtype=numpy.int32), numpy.array([0, 1, 2, 2], dtype=numpy.int32))


_problems, _plain_runs = {}, {}


def _problem(n):
    """(X*, start, lr) of size n, made once."""
    if n not in _problems:
        xs = _oracle.random_walk(n, seed=n)
        _problems[n] = (xs, _oracle.noisy_init(xs), 1.0 / (2 * n))
    return _problems[n]


def _engine(dtype, n, **kw):
    e = HipEngine(n, dtype, **kw)
    e.set_wish_from_coords(_problem(n)[0])
    return e


def _fit(e, k=K):
    """k iterations from the problem's start: (coordinates, stress history)."""
    _, x0, lr = _problem(e.n_bins)
    e.set_coords(x0)
    e.iterate(k, lr)
    return e.get_coords(), e.stress_history()


def _plain(dtype, n, path, k=K):
    """What a fresh engine that saw nothing else computes on `path`; made once, never changed."""
    key = (dtype, n, path, k)
    if key not in _plain_runs:
        e = _engine(dtype, n)
        assert e.iteration_path()[0] == path
        _plain_runs[key] = _fit(e, k)
        e.close()
    return _plain_runs[key]


def _same(got, want):
    assert numpy.array_equal(got[0], want[0]) and numpy.array_equal(got[1], want[1])


# ---- 1. bb_solver_set_maps twice ---------------------------------------------------------------
def _fit_maps(dtype, n, calls):
    """An engine that got set_maps(*c) for every c of calls, then every map's wish block of the
    last call, then K iterations: (coordinates, history, per-map stress, stress)."""
    xs, x0, lr = _problem(n)
    w = _oracle.wish_from_coords(xs)
    e = HipEngine(n, dtype, tiles=TILES)
    for begin, scale in calls:
        e.set_maps(begin, scale)
    begin = calls[-1][0]
    for a, b in zip(begin[:-1], begin[1:]):
        e.set_wish_dense_block(numpy.ascontiguousarray(w[a:b, a:b]), a, "wish", 3.0)
    e.set_coords(x0)
    e.iterate(K, lr)
    out = e.get_coords(), e.stress_history(), e.stress_maps(), e.stress()
    e.close()
    return out


@pytest.mark.parametrize("dtype,n", SIZES)
def test_set_maps_twice_equals_the_last_one_alone(dtype, n, monkeypatch):
    """The tables of the first bb_solver_set_maps are freed and made anew by the second: two
    maps then one, and one then two, each against an engine that got the second call only.
    Unit sweep only: bb_solver_set_maps itself switches the row-owner path off.  Also
    bb_solver_stress of several maps: the sum of bb_solver_stress_maps in index order."""
    monkeypatch.setenv("BB_ROW_OWNER_MAX", "0")
    vw = layout_info(n, dtype)["vw"]
    two, one = ([0, vw, n], [1.0, 0.5]), ([0, n], [0.75])
    for first, second in ((two, one), (one, two)):
        got, want = _fit_maps(dtype, n, [first, second]), _fit_maps(dtype, n, [second])
        assert got[1].size == K * (len(second[0]) - 1)
        for g, w in zip(got, want):
            assert numpy.array_equal(g, w)
        total = got[2][0]
        for v in got[2][1:]:
            total += v
        assert got[3] == total


# ---- 2. bin steps set and cleared ------------------------------------------------------------
@pytest.mark.parametrize("dtype,n", SIZES)
def test_bin_steps_set_cleared_and_set_again(dtype, n, solver_path):
    """bb_solver_set_bin_steps(v) then (NULL) frees the factors: K iterations equal those of an
    engine that never had any.  Setting v again allocates them anew: K more iterations equal
    those of an engine that went the same way and got v once."""
    _, x0, lr = _problem(n)
    v = numpy.random.default_rng(5).uniform(0.5, 1.5, n)
    e = _engine(dtype, n)
    e.set_bin_steps(v)
    e.set_bin_steps(None)
    _same(_fit(e), _plain(dtype, n, solver_path))
    e.set_bin_steps(v)
    e.iterate(K, lr)
    once = _engine(dtype, n)
    _fit(once)
    once.set_bin_steps(v)
    once.iterate(K, lr)
    _same((e.get_coords(), e.stress_history()), (once.get_coords(), once.stress_history()))
    e.close()
    once.close()


# ---- 3. an exchange buffer the caller replaced ---------------------------------------------------
# torch before the library's first call, so that both use one HIP runtime (solver.exchange_tensor):
# a process of its own, all four variants in it.
_EXCHANGE_SCRIPT = r"""
import os, sys
import numpy, torch
sys.path.insert(0, %(root)r)
from blueberry_amd.solver import HipEngine
from tests import _oracle
for dtype, n in %(sizes)r:
    xs = _oracle.random_walk(n, seed=n)
    x0, lr = _oracle.noisy_init(xs), 1.0 / (2 * n)
    for path in ("row_owner", "units"):
        os.environ["BB_ROW_OWNER_MAX"] = "4096" if path == "row_owner" else "0"
        def engine():
            e = HipEngine(n, dtype)
            assert e.iteration_path()[0] == path
            e.set_wish_from_coords(xs)
            e.set_coords(x0)
            return e
        e = engine()
        t = e.exchange_tensor()
        e.grad()
        before = e.read_exchange()
        e.apply(lr)
        e.close()
        torch.cuda.synchronize()
        assert numpy.abs(before).max() > 0
        assert numpy.array_equal(t.cpu().numpy().astype(numpy.float64), before), (dtype, path)
        runs = []
        for _ in range(2):                     # the device is healthy: two more handles agree
            e = engine()
            e.iterate(%(k)d, lr)
            runs.append((e.get_coords(), e.stress_history()))
            e.close()
        assert numpy.array_equal(runs[0][0], runs[1][0]) and numpy.array_equal(runs[0][1], runs[1][1])
        assert numpy.isfinite(runs[0][1]).all() and runs[0][1][-1] < runs[0][1][0]
print("EXCHANGE_OK")
"""


def test_replaced_exchange_buffer_outlives_the_handle():
    """exchange_tensor() replaces the exchange buffer by a torch tensor (the solver's own is
    freed then); after grad, apply and close the tensor is still readable and holds what
    read_exchange returned: the handle does not free memory it was given.  Then new handles fit."""
    script = _EXCHANGE_SCRIPT % {"root": ROOT, "sizes": SIZES, "k": K}
    env = {k: v for k, v in os.environ.items() if k != "BB_ROW_OWNER_MAX"}
    r = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=300,
                       env=env, cwd=ROOT)
    assert "EXCHANGE_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- 4. a peer arena exported, never connected ---------------------------------------------------
@pytest.mark.parametrize("dtype,n", SIZES)
def test_peer_export_without_connect_then_close(dtype, n, solver_path):
    """The one-rank rehearsal stopped half way: the arena is made (bb_solver_peer_export), no
    table, mask, state or counter ever is; close frees what there is, and the next engine fits."""
    e = _engine(dtype, n)
    buf = ctypes.create_string_buffer(_lib.BB_PEER_HANDLE_BYTES)
    _lib.check(e._lib.bb_solver_peer_export(e._h, buf), "bb_solver_peer_export")
    e.close()
    nxt = _engine(dtype, n)
    _same(_fit(nxt), _plain(dtype, n, solver_path))
    nxt.close()


@pytest.mark.parametrize("one_launch", [True, False], ids=["one_launch", "two_launches"])
@pytest.mark.parametrize("dtype,n", SIZES)
def test_peer_link_connected_to_itself_then_close_twice_over(dtype, n, one_launch, monkeypatch):
    """The one-rank rehearsal carried through: export, connect to its own arena (tables, mask,
    state and counter are made), three bb_solver_iterate_peer steps in the given form, close --
    the peer link ends with the handle -- and a second solver on the device does the same.  One
    rank's exchange adds nothing, so both give the bits of three bb_solver_iterate steps of the
    unit sweep (the path the peer exchange steps from) from the same start."""
    monkeypatch.setenv("BB_ROW_OWNER_MAX", "0")
    _, x0, lr = _problem(n)
    want = _plain(dtype, n, "units", 3)
    for _ in range(2):
        e = _engine(dtype, n)
        buf = ctypes.create_string_buffer(_lib.BB_PEER_HANDLE_BYTES)
        _lib.check(e._lib.bb_solver_peer_export(e._h, buf), "bb_solver_peer_export")
        _lib.check(e._lib.bb_solver_peer_connect(e._h, buf.raw), "bb_solver_peer_connect")
        e.peer_set_form(one_launch)
        assert e.peer_form() == ("one launch" if one_launch else "two launches")
        e.set_coords(x0)
        e.iterate_peer(3, lr)
        assert e.peer_status() == 0
        got = e.get_coords(), e.stress_history()
        e.close()
        assert numpy.array_equal(got[0], want[0])
        # (the stress travels through the arena as a (hi, lo) pair of the solver's type: 48 bits
        # of it in fp32, so the history agrees to 2^-48 and is not compared bit for bit)
        assert got[1].shape == (3,) and numpy.abs(got[1] - want[1]).max() <= 2.0 ** -40 * want[1].max()


# ---- 5. timing events and the two measurements on one handle -----------------------------------
@pytest.mark.parametrize("dtype,n", SIZES)
def test_timing_and_measurements_change_no_bit(dtype, n, solver_path):
    """The handle's events (bb_solver_set_timing) and the measurements' own, on one handle, and
    two closes: the stress history is that of an engine without timing."""
    e = _engine(dtype, n)
    e.set_timing(1)
    got = _fit(e, 3)
    t = e.timing()
    assert t["launches"] == 3 and t["grad_ms"] >= 0.0 and t["reduce_ms"] >= 0.0
    assert e.event_gap_ms(2) >= 0.0
    assert e.stream_read_ms(2) > 0.0
    got = (got[0], e.stress_history())
    e.close()
    e.close()
    _same(got, _plain(dtype, n, solver_path, 3))


# ---- 6. a create that fails ----------------------------------------------------------------------
@pytest.mark.parametrize("dtype,n", SIZES)
def test_failed_create_leaves_the_device_usable(dtype, n, solver_path):
    """A tile list out of (J, I) order fails after the handle exists and before its buffers do:
    the half-made handle is torn down, the error text is the create's, the next engine fits."""
    with pytest.raises(ValueError, match=r"bb_solver_create: tile list must be strictly ordered by "
                                         r"\(J, I\) with 0 <= I <= J < n_blocks"):
        HipEngine(n, dtype, tiles=(TILES[0][::-1], TILES[1][::-1]))
    e = _engine(dtype, n)
    _same(_fit(e), _plain(dtype, n, solver_path))
    e.close()


# ---- 7. a group that is refused ------------------------------------------------------------------
@pytest.mark.parametrize("dtype,n", SIZES)
def test_rejected_group_leaves_its_members_usable(dtype, n, solver_path):
    """bb_group_create with a member 1 that was created as rank 0: refused with the text it has
    today, and both members go on as before -- the same stress -- and close."""
    members = [_engine(dtype, n, rank=0, world=2) for _ in range(2)]
    for e in members:
        e.set_coords(_problem(n)[1])
    before = [e.stress() for e in members]
    g = ctypes.c_void_p()
    arr = (ctypes.c_void_p * 2)(*[e._h.value for e in members])
    with pytest.raises(ValueError, match="bb_group_create: member 1 is rank 0 of world 2; member r "
                                         "must be rank r of world 2"):
        _lib.check(members[0]._lib.bb_group_create(g, arr, 2), "bb_group_create")
    assert not g.value
    assert [e.stress() for e in members] == before and before[0] > 0.0
    for e in members:
        e.close()


# ---- 8. triples ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,n", SIZES)
def test_triples_tiles_close_twice_and_empty(dtype, n):
    """DeviceTriples: made, asked for its tiles, closed twice; then one of no rows at all.  (No
    solver in it, so no iteration path to choose.)"""
    res = 5000
    rng = numpy.random.default_rng(8)
    i, j = rng.integers(0, n, 400), rng.integers(0, n, 400)
    t = DeviceTriples(numpy.stack([i * res, j * res, rng.integers(1, 9, 400)], axis=1), res, 0)
    ti, tj = t.tiles(n, dtype)
    vw = layout_info(n, dtype)["vw"]
    want = sorted({(max(a, b) // vw, min(a, b) // vw) for a, b in zip(i.tolist(), j.tolist())})
    assert list(zip(tj.tolist(), ti.tolist())) == want
    t.close()
    t.close()
    empty = DeviceTriples(numpy.zeros((0, 3)), res, 0)
    assert empty.n == 0
    empty.close()


# ---- 9. every owner of a library handle: closed twice, refused afterwards, closed by `with` ------
# The smallest size each exists at: N = 300 fp64 (the narrow layout), a band of seven diagonals
# of whole counts over 300 bins (2,079 triples), 4 sources, d = 301.  A closed handle raises
# ValueError in Python (`_lib.Handle`): the library never sees it.
_RES, _BINS = 5000, 300


def _band_triples():
    i = numpy.repeat(numpy.arange(_BINS), 7)
    j = i + numpy.tile(numpy.arange(7), _BINS)
    keep = j < _BINS
    i, j = i[keep], j[keep]
    return numpy.stack([i * float(_RES), j * float(_RES), 1.0 + (i * 7 + j) % 9], axis=1)


def _make_engine():
    return _engine("float64", _BINS), lambda e: e.layout()["n_bins"] == _BINS


def _make_group():
    from blueberry_amd.solver import GroupEngine
    xs, x0, lr = _problem(_BINS)
    g = GroupEngine(_BINS, "float64", [0, 0])
    g.set_wish_from_coords(xs)
    g.set_coords(x0)

    def call(g):
        g.iterate(1, lr)
        g.sync()
        return True
    return g, call


def _make_triples():
    t = _band_triples()
    return DeviceTriples(t, _RES, 0), lambda d: d.pairs(_BINS) == t.shape[0]


def _make_rows():
    t = DeviceTriples(_band_triples(), _RES, 0)
    rows = t.shortest_paths(_BINS, [0, 100, 200, 299])
    t.close()                                      # (the rows own their memory)
    return rows, lambda r: r.reached().tolist() == [_BINS] * 4


def _make_matrix():
    import blueberry_amd as bb
    cm = bb.ContactMap.from_triples(_band_triples(), _RES, _BINS)
    return cm._resident(), lambda m: m.d == _BINS + 1


def _make_results():
    import blueberry_amd as bb
    from blueberry_amd import fithic
    cm = bb.ContactMap.from_triples(_band_triples(), _RES, _BINS)
    n_reads = 1e4
    prior = 8.0 / (numpy.arange(_BINS) + 1.0) / n_reads
    res = fithic.significance_list(cm, _BINS, 1, 6, numpy.ones(_BINS), None, prior, n_reads)
    res.map_ = cm                                  # (the map lives as long as its list)
    return res, lambda r: 0 < r.size()[0] <= _band_triples().shape[0] - _BINS


@pytest.mark.parametrize("make", [_make_engine, _make_group, _make_triples, _make_rows, _make_matrix,
                                  _make_results], ids=lambda f: f.__name__[6:])
def test_every_handle_owner_closes_twice_refuses_then_and_closes_on_exit(make):
    h, call = make()
    members = list(getattr(h, "members", ()))
    assert isinstance(h, _lib.Handle) and h._h
    assert call(h)
    h.close()
    h.close()
    assert not h._h and not any(m._h for m in members)
    with pytest.raises(ValueError, match="closed"):
        call(h)
    with make()[0] as again:
        assert again._h
    assert not again._h
