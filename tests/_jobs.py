"""Test-only: one job of `world` ranks over a gloo group, a spawned process each, that runs a
worker once and hands back one value per rank.  (tests/_ranks.py is the other process helper:
long-lived ranks with a HipEngine each, driven call by call.)

    values = run_ranks(worker, world, *args)          # values[rank]

A worker is a module-level function `worker(rank, world, *args)`; what it returns comes back.
Whatever goes wrong -- a worker raises, a process dies, a rank gives no answer -- run_ranks
raises and names the rank, and no process it started is alive when it returns or raises.
Never imported by the package."""
import importlib
import multiprocessing
import os
import queue
import signal
import socket
import sys
import time
import traceback

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POLL_S = 0.1               # between two looks at the children
LAST = []                  # the processes of the latest run_ranks call, in rank order


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


@pytest.fixture
def one_rank_group(monkeypatch):
    """A gloo group of one rank in the test process itself (no process is started), for tests
    of what the solver decides from torch.distributed's state; BB_COMM is unset."""
    import torch.distributed as dist
    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", str(free_port()))
    monkeypatch.delenv("BB_COMM", raising=False)
    dist.init_process_group("gloo", rank=0, world_size=1)
    yield dist
    dist.destroy_process_group()


def _rank_main(rank, world, port, module, name, args, env, finish, q):
    """The spawn target.  The worker travels by name and is imported only after `env` is
    applied, so that nothing of the package is imported before."""
    dist = None
    try:
        if ROOT not in sys.path:
            sys.path.insert(0, ROOT)
        for key, value in (env or {}).items():
            if value is None:
                os.environ.pop(key, None)
            else:
                os.environ[key] = value
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        import torch.distributed as dist
        dist.init_process_group("gloo", rank=rank, world_size=world)
        worker = getattr(importlib.import_module(module), name)
        answer = ("ok", rank, worker(rank, world, *args))
    except Exception:                              # noqa: BLE001 -- reported to the parent
        answer = ("err", rank, traceback.format_exc())
    q.put(answer)
    if finish == "exit":
        q.close()
        q.join_thread()      # the answer must have left before the hard exit
        os._exit(0)          # a collective nobody will ever complete may still be pending
    if answer[0] == "ok":
        dist.barrier()
        dist.destroy_process_group()


def _ended(procs, ranks):
    """What became of those of `ranks` whose process is gone: a text, '' if all are alive."""
    out = []
    for r in ranks:
        code = procs[r].exitcode
        if code is None:
            continue
        how = "exited with code %d" % code
        if code < 0:                               # a negative code is a signal
            try:
                how = "was ended by signal %d (%s)" % (-code, signal.Signals(-code).name)
            except ValueError:
                how = "was ended by signal %d" % -code
        out.append("the process of rank %d %s without an answer" % (r, how))
    return "; ".join(out)


def run_ranks(worker, world, *args, timeout=240, env=None, finish="barrier"):
    """Run worker(rank, world, *args) on `world` gloo ranks; the list of what they returned,
    index = rank.  `timeout` (s) bounds the wait for each next answer.  `env`: names set in
    every rank before the package is imported (None unsets one).  finish='barrier': the ranks
    meet in a barrier and take the group down; 'exit': they leave by os._exit(0) at once."""
    assert finish in ("barrier", "exit")
    ctx = multiprocessing.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_rank_main, args=(r, world, port, worker.__module__,
                                                  worker.__qualname__, args, env, finish, q))
             for r in range(world)]
    LAST[:] = procs
    values, done = {}, False
    try:
        for p in procs:
            p.start()
        deadline, gone = time.monotonic() + timeout, ""
        while len(values) < world:
            try:
                status, rank, value = q.get(timeout=POLL_S)
            except queue.Empty:
                silent = [r for r in range(world) if r not in values]
                dead = _ended(procs, silent)
                if dead and dead == gone:
                    raise RuntimeError(dead)
                gone = dead      # one more look: an answer sent just before the exit is in the pipe
                if not dead and time.monotonic() > deadline:
                    raise TimeoutError("no answer within %d s from rank(s) %s"
                                       % (timeout, ", ".join(map(str, silent))))
                continue
            if status == "err":
                time.sleep(POLL_S)       # a peer that died just before is the likelier cause
                dead = _ended(procs, [r for r in range(world) if r not in values and r != rank])
                raise RuntimeError("rank %d failed%s:\n%s"
                                   % (rank, " (%s)" % dead if dead else "", value))
            values[rank] = value
            deadline = time.monotonic() + timeout
        done = True
        return [values[r] for r in range(world)]
    finally:
        # ranks that answered are on their way out; after a failure the others may sit in a
        # collective for good
        end = time.monotonic() + (60 if done else 1)
        for p in procs:
            if p.pid is not None:
                p.join(max(0.0, end - time.monotonic()))
        for p in procs:
            if p.is_alive():
                p.kill()
        for p in procs:
            if p.pid is not None:
                p.join(30)
