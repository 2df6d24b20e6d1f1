"""How the ranks of a torch.distributed job sum their partial gradients: the transports, the
choice between them (`select_exchange`, with bench.py's timed trial) and the iteration loop on
top (`run_iterations`).  Collective throughout; everything an engine must offer is duck-typed."""
import os

import numpy

from .ranks import all_ranks


def allreduce_exchange(t):
    """Sum a device-resident exchange tensor over all ranks, in place: one
    all-reduce of 3*n_pad+2 elements (backend nccl = RCCL, over xGMI)."""
    import torch.distributed as dist
    dist.all_reduce(t, op=dist.ReduceOp.SUM)


def allreduce_exchange_host(eng):
    """The same sum for a host-memory collective (backend gloo: CPU rehearsals,
    tests, 2 ranks sharing one GPU): read the buffer through the C-ABI, reduce
    on the host in float64, write it back.  Transport only -- the kernels on
    either side are the same ones the RCCL path runs."""
    import torch
    import torch.distributed as dist
    host = torch.from_numpy(eng.read_exchange())
    dist.all_reduce(host, op=dist.ReduceOp.SUM)
    eng.write_exchange(host.numpy())


_TRIAL_PEER_TIMEOUT_MS = 2000
_TRIAL_SYNC_TIMEOUT_MS = int(os.environ.get("BB_TRIAL_SYNC_TIMEOUT_MS", "30000"))


def _trial_leg(eng, name, step, lr, x0, iters):
    """One transport's trial run from the start x0: one step (coordinates kept for the
    agreement check), ten more to warm up, `iters` timed.  After EVERY stage the ranks
    agree on whether all of them got through it; the first stage that failed anywhere
    ends the leg on every rank, so nobody enters a collective that a peer has left.
    Returns (ok, coordinates after one step, seconds per iteration)."""
    import time
    import torch.distributed as dist
    box = {}

    def stage(fn):
        try:
            fn()
            ok = True
        except Exception as exc:                 # this transport is just not used
            eng._comm_trial_error = "%s: %s" % (name, exc)
            ok = False
        return all_ranks(ok)

    def settle():
        # bounded: a collective that a peer never joined must end the leg, not the job
        bounded = getattr(eng, "sync_timeout", None)
        if bounded:
            bounded(_TRIAL_SYNC_TIMEOUT_MS)
        else:
            eng.sync()
        if name == "peer":
            eng.peer_status()                    # raises when a wait ran into its limit

    def first():
        eng.set_coords(x0)
        step(1, lr)
        settle()
        box["x1"] = eng.get_coords()

    def warm():
        step(10, lr)
        settle()

    def timed():
        t0 = time.perf_counter()
        step(iters, lr)
        settle()
        box["dt"] = (time.perf_counter() - t0) / iters
        box["xk"] = eng.get_coords()             # after 1 + 10 + iters steps (outside the clock)

    for k, fn in enumerate((first, warm, timed)):
        if k == 2:
            dist.barrier()
        if not stage(fn):
            return False, None, float("inf")
    # coordinates after the FIRST step and after the LAST: a transport that delivers a stale
    # or torn partial now and then shows in the second even when the first step went well
    return True, (box["x1"], box["xk"]), box["dt"]


def comm_reuse(eng):
    """Borrow the communicator an earlier solver of this job made: the library keeps one
    per (device, rank, world) for the life of the process, so only the first multi-rank
    fit() pays ncclCommInitRank (0.1-1 s; round 2 made and destroyed one per fit).
    Collective, and the same on every rank by construction: the ranks first agree that
    EVERY one of them holds a free cached communicator, then that every attach worked;
    otherwise nobody uses the cache and `comm_setup` makes a fresh one everywhere."""
    if hasattr(eng, "_comm_generation"):
        # ... and that it is the SAME communicator on all of them: the cache is keyed by
        # (device, rank, world) only, and a rank can hold one of another generation -- made
        # while a peer's earlier solver still held the previous one, or by an earlier process
        # group of the same size.  Attaching those would hang the first all-reduce.
        import torch.distributed as dist
        gens = [None] * dist.get_world_size()
        dist.all_gather_object(gens, eng._comm_generation())
        if gens[0] == 0 or any(g != gens[0] for g in gens):
            return False
    elif not all_ranks(eng._comm_cached()):
        return False
    ok = eng._comm_attach()
    if not all_ranks(ok):
        if ok:
            eng._comm_detach()
        return False
    return True


def _comm_get(eng):
    """The library's communicator for this engine: the one an earlier fit() of this job
    left in the library's cache (`comm_reuse`), else a new one (`comm_setup`).  Collective."""
    if hasattr(eng, "_comm_cached") and comm_reuse(eng):
        return True
    return eng.comm_setup()


def _exchange_state(eng):
    """The transport `select_exchange` chose for this engine ('group' for a GroupEngine), or
    None: nothing chosen yet, or an engine that never sums over ranks."""
    return getattr(eng, "_comm_state", None)


def select_exchange(eng, lr, trial=False):
    """Decide, once per engine and identically on every rank, how the partial
    gradients are summed over the ranks.  Collective.

    BB_COMM = auto (default) | peer | rccl | torch | host
      peer   one-shot exchange inside the solver's own kernels (IPC-mapped arenas)
      rccl   the library's own RCCL communicator, all-reduce enqueued from C
      torch  torch.distributed all-reduce on a tensor aliasing the exchange buffer
      host   exchange buffer staged through host memory (gloo / CPU rehearsals)
    auto on an RCCL job means rccl (torch if the communicator cannot be made).  With
    `trial` true -- bench.py, or BB_COMM_TRIAL=1 -- and the coordinates just set, auto
    also sets up peer and runs a few iterations through both from the same start
    (`_exchange_trial`).  The outcome is kept in eng._comm_state / eng._comm_trial."""
    if _exchange_state(eng):
        return eng._comm_state
    want = os.environ.get("BB_COMM", "auto")
    if want not in ("auto", "peer", "rccl", "torch", "host"):
        raise ValueError("BB_COMM must be auto, peer, rccl, torch or host, not %r" % want)
    trial = bool(trial) or os.environ.get("BB_COMM_TRIAL") == "1"
    state = _exchange_untried(eng, want, trial)
    if state is None:
        have_rccl = _comm_get(eng)
        if eng.peer_setup() and (have_rccl or hasattr(eng, "exchange_tensor")):
            state = _exchange_trial(eng, lr, have_rccl)
        else:
            state = "rccl" if have_rccl else "torch"
    eng._comm_state = state
    return state


def _exchange_untried(eng, want, trial):
    """The transport where no trial decides it, or None where one does (auto on an RCCL job
    with `trial`)."""
    import torch.distributed as dist
    native = hasattr(eng, "peer_setup")
    nccl = dist.get_backend() == "nccl"
    if not native or want == "host" or (not nccl and want != "peer"):
        return "host"
    if want == "peer":
        if not eng.peer_setup():
            raise RuntimeError("BB_COMM=peer but the peer exchange could not be set up: %s"
                               % eng._peer_error)
        # No trial has compared this exchange with RCCL: keep the two-launch form, which
        # applies a step whole or not at all and whose flags are ordered by release / acquire.
        # The one-launch form (data as its own flag, no fences) is taken where a trial has
        # validated it against RCCL on this very job, or on request (BB_PEER_FUSED=1).
        if not trial and os.environ.get("BB_PEER_FUSED") is None and hasattr(eng, "peer_set_form"):
            eng.peer_set_form(False)
        return "peer"
    if want == "torch":
        return "torch"
    if want == "rccl" or not trial:
        return "rccl" if _comm_get(eng) else "torch"
    return None


def _exchange_trial(eng, lr, have_rccl):
    """Run the peer exchange against a reference from the same start and return the one to
    use: peer only if its coordinates agree with the reference's and it is faster on the
    slowest rank; the start is restored afterwards.  The reference, which also runs if peer
    loses, is the library's communicator or -- when that could not be made --
    torch.distributed's all-reduce on the exchange buffer.  Every stage ends with an
    agreement between the ranks (`_trial_leg`), and the peer waits are cut to 2 s while it
    runs, so a transport that fails on one rank is dropped by all of them instead of leaving
    the others inside a collective.  Collective; the figures go to eng._comm_trial."""
    import torch.distributed as dist
    ref = "rccl" if have_rccl else "torch"
    ref_step = _stepper(eng, ref)
    x0 = eng.get_coords()
    set_limit = getattr(eng, "peer_set_timeout", None)
    if set_limit:
        set_limit(_TRIAL_PEER_TIMEOUT_MS)
    eng._comm_trial_error = None

    def reference_leg():
        run = _trial_leg(eng, ref, ref_step, lr, x0, 30)
        if have_rccl and not run[0] and hasattr(eng, "comm_abort"):
            # the library's communicator is suspect (this rank may still sit in a
            # collective a peer never joined): abort it -- every rank does,
            # the leg's outcome is shared -- so that the stream drains again
            try:
                eng.comm_abort()
            except Exception as exc:
                eng._comm_trial_error = "%s; abort: %s" % (eng._comm_trial_error, exc)
        return run

    runs = {"reference": reference_leg()}
    runs["peer"] = _trial_leg(eng, "peer", eng.iterate_peer, lr, x0, 30)
    if runs["reference"][0] and runs["peer"][0]:
        # the leg that runs first is timed on a chip whose clocks have not settled
        # (a block right after idle runs 4-19 % slow): the reference gets a
        # second timing behind the peer leg and keeps its better one.  (Leg outcomes
        # are agreed between the ranks, so every rank takes this branch or none.)
        again = reference_leg()
        if again[0]:
            runs["reference"] = (True, runs["reference"][1], min(runs["reference"][2], again[2]))
        else:
            runs["reference"] = again
    if set_limit and runs["peer"][0]:
        set_limit(int(os.environ.get("BB_PEER_TIMEOUT_MS", "10000")))
    eng.set_coords(x0)
    scale = float(numpy.abs(x0).max() + 1e-30)
    # one step: 1e-4 (the transports add the ranks' partials in different orders); the
    # whole leg, 41 steps: 1e-3 -- far above what the order of a sum does over that
    # many steps in fp32 (1e-5), far below what a lost or torn partial does
    agree = bool(runs["reference"][0] and runs["peer"][0]
                 and numpy.allclose(runs["reference"][1][0], runs["peer"][1][0], rtol=1e-4,
                                    atol=1e-6 * scale)
                 and numpy.allclose(runs["reference"][1][1], runs["peer"][1][1], rtol=1e-3,
                                    atol=1e-5 * scale))
    mine = (agree, runs["reference"][2], runs["peer"][2])
    every = [None] * eng.world
    dist.all_gather_object(every, mine)
    t_ref = max(e[1] for e in every)
    t_peer = max(e[2] for e in every)
    # the reference is the plain path: the peer exchange has to win by more than the
    # trial's own noise (3 %), not by a coin flip
    use_peer = all(e[0] for e in every) and t_peer < 0.97 * t_ref
    ms = lambda t: t * 1e3 if numpy.isfinite(t) else None
    eng._comm_trial = {"agree": all(e[0] for e in every), "reference": ref,
                       "rccl_ms": ms(t_ref),      # (the reference leg's time)
                       "peer_ms": ms(t_peer),
                       "error": eng._comm_trial_error}
    if use_peer:
        return "peer"
    return ref if runs["reference"][0] else "torch"


def _stepper(eng, state):
    """The callable (k, lr) that runs k iterations of `eng` with the transport `state`
    summing the ranks' partial gradients."""
    if state == "peer":
        return eng.iterate_peer
    if state == "rccl":
        return eng.iterate_dist

    def step(k, lr):
        # per iteration: local partial gradient -> sum over ranks -> identical update
        t = eng.exchange_tensor() if state == "torch" else None
        for _ in range(k):
            eng.grad()
            if t is None:
                allreduce_exchange_host(eng)
            else:
                allreduce_exchange(t)
            eng.apply(lr)
    return step


def run_iterations(eng, n_iter, lr, world):
    """n_iter solver iterations on an engine whose inputs are set.

    world == 1: the whole loop is enqueued by one C call.  world > 1: per
    iteration, local partial gradient -> sum over ranks -> identical update on
    every rank, so the replicas of X stay identical; `select_exchange` picks the
    transport."""
    if world == 1:
        eng.iterate(n_iter, lr)
    else:
        _stepper(eng, select_exchange(eng, lr))(n_iter, lr)
