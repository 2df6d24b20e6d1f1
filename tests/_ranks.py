"""Test-only: ranks of one job, each a HipEngine in a process started for it, connected
through the peer exchange as a job of several processes connects them.

Ranks that wait for one another on the device cannot be streams of one process at will:
the HIP runtime gives a process only a few hardware queues, and a rank's kernel that waits
for a peer would sit in front of that peer's kernel in a shared queue.  So every rank gets a
process of its own, or -- where a job has more ranks than processes may hold the GPU at
once -- two ranks share one: the first on the stream its engine made (created while the
process has at most one other queue, so it gets one of its own) and the second on the
device's null stream, which holds the other queue.  Two ranks of one process still share
the null stream with the host copies the library makes, so calls that read back while their
peers run ahead (the spectral start with a tolerance) are for ranks of their own processes
only (`shares_process`).  Processes are spawned, never forked from a test process that has
opened the GPU.  Never imported by the package."""
import multiprocessing
import os
import sys
import threading

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_RANK_PROCESSES = 4     # with the test process (and a tool between the two): at most 6
                           # processes hold the GPU at once


def _call(eng, name, *args, **kwargs):
    return getattr(eng, name)(*args, **kwargs)


def _serve(eng, conn):
    while True:
        msg = conn.recv()
        if msg is None:
            break
        fn, args, kwargs = msg
        try:
            conn.send(("ok", fn(eng, *args, **kwargs)))
        except BaseException as exc:               # noqa: BLE001 -- reported to the driver
            conn.send(("err", exc))
    eng.close()
    conn.send(("ok", None))


def _host_main(conns, n, dtype, ranks, world, tiles):
    """A process holding `ranks` (one or two): builds their engines, then serves each
    rank's requests, fn(engine, *args, **kwargs), on a thread of its own."""
    sys.path.insert(0, ROOT)
    from blueberry_amd import _lib
    from blueberry_amd.solver import HipEngine
    engs = []
    for i, (conn, rank) in enumerate(zip(conns, ranks)):
        try:
            eng = HipEngine(n, dtype, rank=rank, world=world, tiles=tiles)
            if i > 0:
                _lib.check(eng._lib.bb_solver_set_stream(eng._h, None), "bb_solver_set_stream")
            engs.append(eng)
        except BaseException as exc:               # noqa: BLE001
            for c in conns:
                c.send(("err", exc))
            return
    for conn in conns:
        conn.send(("ok", None))
    threads = [threading.Thread(target=_serve, args=(e, c)) for e, c in zip(engs, conns)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()


LIVE = []


class Rank(object):
    """One rank's HipEngine in a rank process, driven from here: its methods are called as
    the engine's would be, `run(fn, *args)` runs fn(engine, *args) there."""

    def __init__(self, host, conn, rank, shares_process):
        self._host, self._conn = host, conn
        self.rank, self.shares_process = rank, shares_process
        LIVE.append(self)

    def _answer(self, timeout=600):
        if not self._conn.poll(timeout):
            self._host.kill()
            raise TimeoutError("rank %d gave no answer within %d s" % (self.rank, timeout))
        try:
            status, value = self._conn.recv()
        except EOFError:
            self._host.kill()
            raise RuntimeError("the process of rank %d ended without an answer (exit code %s)"
                               % (self.rank, self._host.exitcode))
        if status == "err":
            raise value
        return value

    def run(self, fn, *args, **kwargs):
        self._conn.send((fn, args, kwargs))
        return self._answer()

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        return lambda *args, **kwargs: self.run(_call, name, *args, **kwargs)

    def close(self):
        if self not in LIVE:
            return
        LIVE.remove(self)
        try:
            self._conn.send(None)
            self._answer(120)
        except (OSError, RuntimeError):
            pass                                   # the process had ended already
        if not any(r._host is self._host for r in LIVE):
            self._host.join(60)
            self._host.kill()
            self._host.join(30)


def close_all():
    while LIVE:
        LIVE[-1].close()


@pytest.fixture(autouse=True)
def no_rank_process_outlives_its_test():
    """For the test modules that start ranks to import: autouse in a module that holds it."""
    yield
    close_all()


def start(world, n, dtype, tiles=None):
    """`world` ranks, one process each, or two a process where world exceeds
    MAX_RANK_PROCESSES (at most 2 * MAX_RANK_PROCESSES ranks)."""
    if world > 2 * MAX_RANK_PROCESSES:
        raise ValueError("at most %d ranks" % (2 * MAX_RANK_PROCESSES))
    ctx = multiprocessing.get_context("spawn")
    n_proc = min(world, MAX_RANK_PROCESSES)
    groups = [list(range(world))[p::n_proc] for p in range(n_proc)]
    out = [None] * world
    for ranks in groups:
        pipes = [ctx.Pipe() for _ in ranks]
        host = ctx.Process(target=_host_main,
                           args=([c for _, c in pipes], n, dtype, ranks, world, tiles), daemon=True)
        host.start()
        for (_, c) in pipes:
            c.close()
        for (p, _), r in zip(pipes, ranks):
            out[r] = Rank(host, p, r, len(ranks) > 1)
    for r in out:
        r._answer()
    return out


def _peer_export(eng):
    import ctypes
    from blueberry_amd import _lib
    buf = ctypes.create_string_buffer(_lib.BB_PEER_HANDLE_BYTES)
    _lib.check(eng._lib.bb_solver_peer_export(eng._h, buf), "export")
    return buf.raw


def _peer_connect(eng, blobs):
    from blueberry_amd import _lib
    _lib.check(eng._lib.bb_solver_peer_connect(eng._h, blobs), "connect")


def connect(ranks):
    """Connect the ranks' receive arenas: the handles of all, in rank order, to every rank."""
    blobs = b"".join(r.run(_peer_export) for r in ranks)
    for r in ranks:
        r.run(_peer_connect, blobs)


def peer_ranks(world, n, dtype, tiles=None):
    ranks = start(world, n, dtype, tiles)
    connect(ranks)
    return ranks
