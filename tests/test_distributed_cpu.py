"""CPU, world_size 2 over gloo: the N>1 path of the solver and of the band
count, with one rank's compute played by the oracle (tests/_engines.py) and
everything else -- unit partition, exchange-buffer layout, the per-iteration
all-reduce, the identical update on every rank -- the product's own code."""
import numpy
import pytest

from tests._jobs import one_rank_group, run_ranks         # noqa: F401 -- a fixture


def _worker(rank, world, n, k, dtype):
    import blueberry_amd as bb
    from blueberry_amd.band import allreduce_count, band_row_share
    from tests import _oracle
    from tests._engines import OracleEngine

    xs = _oracle.random_walk(n)
    w = _oracle.wish_from_coords(xs)
    x0 = _oracle.noisy_init(xs)
    s = bb.StructureSolver(n_iter=k, dtype=dtype, kind="wish", engine=OracleEngine)
    s.fit(w, init=x0)                      # distributed=None: picks up the gloo job
    # spectral start: the per-rank matvec shares are summed over the ranks
    sp = bb.StructureSolver(n_iter=1, dtype=dtype, kind="wish", engine=OracleEngine,
                            init="spectral").fit(w)
    assert sp.stress_[0] < 1e-6 * s.stress_[0], (sp.stress_[0], s.stress_[0])

    r = _oracle.golden("band_count")["in_gappy_n1000"]
    a, b = band_row_share(r.shape[0], rank, world)
    total = allreduce_count(_oracle.load().count_band_regions_rows(r, a, b))
    return s.structure_, s.stress_, total


@pytest.mark.parametrize("world,dtype", [(2, "float32"), (2, "float64"), (3, "float32")])
def test_sharded_solve_equals_single_process_oracle(oracle, world, dtype):
    from tests import _oracle
    n, k = 700, 4
    results = run_ranks(_worker, world, n, k, dtype, timeout=240)

    xs = _oracle.random_walk(n)
    w = _oracle.wish_from_coords(xs)
    X_ref, h_ref = oracle.solve(w, _oracle.noisy_init(xs), k, 1.0 / (2 * n))
    band_ref = int(_oracle.golden("band_count")["out_gappy_n1000"])
    for X, hist, band_total in results:
        assert numpy.abs(X - X_ref).max() < 1e-11 * numpy.abs(X_ref).max()
        assert numpy.abs(hist / h_ref - 1).max() < 1e-11
        assert band_total == band_ref                      # integer all-reduce: exact
    # every rank applied the identical update: replicas are bit-identical
    for X, hist, _ in results[1:]:
        assert numpy.array_equal(X, results[0][0]) and numpy.array_equal(hist, results[0][1])


# ---- degree_steps on several ranks: the degrees are summed over the ranks ----------------
def _degree_worker(rank, world, n, k):
    import blueberry_amd as bb
    from tests._engines import OracleEngine
    w, x0 = _holey_map(n)
    s = bb.StructureSolver(n_iter=k, dtype="float64", kind="wish", engine=OracleEngine,
                           degree_steps=True).fit(w, init=x0)
    return s.structure_, s.stress_, s.lr_


def _holey_map(n):
    """Two dense blocks of unequal size (5 : 1) joined by a narrow band."""
    from tests import _oracle
    xs = _oracle.random_walk(n)
    w = _oracle.wish_from_coords(xs)
    i, j = numpy.indices((n, n))
    cut = (5 * n) // 6
    keep = ((i < cut) & (j < cut)) | ((i >= cut) & (j >= cut)) | (numpy.abs(i - j) <= 30)
    return numpy.where(keep, w, 0.0), _oracle.noisy_init(xs)


def test_degree_steps_on_two_ranks_equal_one_process(oracle):
    """StructureSolver(degree_steps=True) on 2 gloo ranks: every rank counts the degrees of
    its own units, the counts are summed over the ranks, every rank sets the same factors
    and step; the result is the one-process run and the oracle loop with those factors."""
    import blueberry_amd as bb
    from blueberry_amd.solver import degree_step_factors
    from tests._engines import OracleEngine
    n, k, world = 600, 6, 2
    results = run_ranks(_degree_worker, world, n, k, timeout=240)
    w, x0 = _holey_map(n)
    deg = (w > 0).sum(axis=0)
    lr, scale = degree_step_factors(deg)
    assert scale.max() > 3.0
    X, hist = x0.copy(), []
    for _ in range(k):
        s_, g = oracle.stress_grad(w, X)
        X = X - lr * scale[:, None] * g
        hist.append(s_)
    one = bb.StructureSolver(n_iter=k, dtype="float64", kind="wish", engine=OracleEngine,
                             distributed=False, degree_steps=True).fit(w, init=x0)
    plain = bb.StructureSolver(n_iter=k, dtype="float64", kind="wish", engine=OracleEngine,
                               distributed=False).fit(w, init=x0)
    assert one.lr_ == lr and numpy.abs(one.stress_ / numpy.array(hist) - 1).max() < 1e-12
    assert one.stress_[-1] < plain.stress_[-1]
    for Xr, hr, lr_r in results:
        assert lr_r == lr
        assert numpy.abs(hr / numpy.array(hist) - 1).max() < 1e-11
        assert numpy.abs(Xr - X).max() < 1e-11 * numpy.abs(X).max()
    assert numpy.array_equal(results[0][0], results[1][0])


# ---- weighted stress on several ranks: the weighted degrees are summed in float64 -------------
def _weighted_worker(rank, world, n, k):
    import blueberry_amd as bb
    from tests._engines import OracleEngine
    from tests.test_weighted_stress import count_map, start, wish_of
    C = count_map(n, seed=31)
    x0 = start(n, wish_of(C, "float64"))
    s = bb.StructureSolver(n_iter=k, dtype="float64", engine=OracleEngine, weight_power=2,
                           degree_steps=True).fit(C, init=x0)
    return s.structure_, s.stress_, s.lr_


@pytest.mark.parametrize("world", [2, 3])
def test_weighted_degree_steps_on_several_ranks_equal_one_process(oracle, world):
    """StructureSolver(weight_power=2, degree_steps=True) on gloo ranks: every rank sums the
    weights delta^-2 of its own units' pairs, the float64 sums are added over the ranks, and
    every rank takes lr = 1 / (2 max s) and the factors max s / s_i.  The result is the
    one-process run and the weighted oracle loop with those steps."""
    import blueberry_amd as bb
    from tests._engines import OracleEngine
    from tests.test_weighted_stress import count_map, start, weights, wish_of
    n, k = 600, 6
    results = run_ranks(_weighted_worker, world, n, k, timeout=240)
    C = count_map(n, seed=31)
    W = wish_of(C, "float64")
    x0 = start(n, W)
    s = weights(W, 2).sum(1)
    lr, scale = 1.0 / (2.0 * s.max()), numpy.where(s > 0, s.max() / numpy.where(s > 0, s, 1), 1.0)
    assert scale.max() > 2.0                       # the steps differ from bin to bin
    X, hist = oracle.solve_weighted(W, x0, k, lr, 2, bin_scale=scale)
    one = bb.StructureSolver(n_iter=k, dtype="float64", engine=OracleEngine, distributed=False,
                             weight_power=2, degree_steps=True).fit(C, init=x0)
    assert abs(one.lr_ / lr - 1) < 1e-14
    assert numpy.abs(one.stress_ / hist - 1).max() < 1e-12
    assert numpy.abs(one.structure_ - X).max() < 1e-12 * numpy.abs(X).max()
    assert numpy.all(numpy.diff(one.stress_) <= 0.0)
    for Xr, hr, lr_r in results:
        assert abs(lr_r / one.lr_ - 1) < 1e-14
        assert numpy.abs(hr / one.stress_ - 1).max() < 1e-11
        assert numpy.abs(Xr - one.structure_).max() < 1e-11 * numpy.abs(X).max()
    for Xr, hr, _ in results[1:]:
        assert numpy.array_equal(Xr, results[0][0]) and numpy.array_equal(hr, results[0][1])


# ---- init='spectral' on several ranks: which form runs, and that the ranks agree --------
def _spectral_worker(rank, world, n, fail_rank):
    """fit(init='spectral') on `world` gloo ranks with an engine that HAS a device-resident
    start and a transport that sums on the device (played: _comm_state = 'peer').  The
    device form must be tried after the exchange is chosen, and if it is refused anywhere
    (RankDeficient on `fail_rank`) EVERY rank must take the host-driven start."""
    import blueberry_amd as bb
    from blueberry_amd import solver
    from tests import _oracle
    from tests._engines import OracleEngine

    log = []
    host_form = solver.spectral_init

    def counted_host_form(*a, **k):
        log.append("host")
        return host_form(*a, **k)

    class Eng(OracleEngine):
        def spectral_init_device(self, n_iter, v0, tol=0.0):
            assert self._comm_state == "peer", "the exchange must be chosen first"
            log.append("device")
            x = host_form(self, self.n_bins, self.world, n_iter=n_iter, seed=0, tol=tol)   # collective
            if rank == fail_rank:
                raise solver.RankDeficient("the iterate lost rank (scripted)")
            self.set_coords(x)

        def peer_status(self):
            return 0

        def iterate_peer(self, k, lr):
            for _ in range(k):
                self.grad()
                solver.allreduce_exchange_host(self)
                self.apply(lr)

    def fake_select(eng, lr, trial=False):
        eng._comm_state = "peer"
        return "peer"

    solver.select_exchange = fake_select
    solver.spectral_init = counted_host_form
    xs = _oracle.random_walk(n)
    w = _oracle.wish_from_coords(xs)
    s = bb.StructureSolver(n_iter=2, dtype="float64", kind="wish", engine=Eng,
                           init="spectral").fit(w)
    return log, s.structure_, s.stress_


@pytest.mark.parametrize("fail_rank", [None, 1])
def test_multi_rank_spectral_start_control_flow(fail_rank):
    from tests import _oracle
    n, world = 300, 2
    results = run_ranks(_spectral_worker, world, n, fail_rank, timeout=240)
    for r in results:
        # the device form is tried once everywhere; refused anywhere -> host form everywhere
        assert r[0] == (["device"] if fail_rank is None else ["device", "host"])
    w = _oracle.wish_from_coords(_oracle.random_walk(n))
    for _, X, hist in results:
        assert numpy.abs(_oracle.wish_from_coords(X) - w).max() < 1e-6 * w.max()
    assert numpy.array_equal(results[0][1], results[1][1])         # replicas identical


# ---- fit_many on several ranks: every rank solves maps of its own ----------------------------
def _many_worker(rank, world):
    import blueberry_amd as bb
    from tests import _oracle
    from tests._engines import OracleEngine
    sizes = [300, 90, 640, 200, 515]
    mats = [_oracle.wish_from_coords(_oracle.random_walk(n, seed=q_)) for q_, n in enumerate(sizes)]
    s = bb.StructureSolver(n_iter=3, dtype="float64", kind="wish", seed=2,
                           engine=OracleEngine).fit_many(mats)      # picks up the gloo job
    # the options travel to the per-rank solvers: a step per bin from each map's degrees
    holes = []
    for q_, m in enumerate(mats[:3]):
        keep = numpy.triu(numpy.random.default_rng(q_).random(m.shape) < 0.3, 1)
        keep |= numpy.triu(numpy.ones(m.shape, dtype=bool), 1) & ~numpy.triu(numpy.ones(m.shape, dtype=bool), 2)
        holes.append(numpy.where(keep | keep.T, m, 0.0))
    d = bb.StructureSolver(n_iter=3, dtype="float64", kind="wish", seed=2, engine=OracleEngine,
                           degree_steps=True).fit_many(holes)
    return s.structures_, s.stresses_, s.ranks_of_maps_, d.lrs_, d.stresses_


def test_fit_many_deals_the_maps_to_the_ranks(oracle):
    """Several GPUs: the maps are independent, so every rank solves maps of its own (dealt by
    size) and all ranks get all results -- equal to the oracle's solve of each map."""
    from tests import _oracle
    results = run_ranks(_many_worker, 2, timeout=240)
    sizes = [300, 90, 640, 200, 515]
    owners = results[0][2]
    assert owners == results[1][2] and set(owners) == {0, 1}
    assert owners[2] != owners[4]                    # the two largest maps go to different ranks
    for m, n in enumerate(sizes):
        w = _oracle.wish_from_coords(_oracle.random_walk(n, seed=m))
        x0 = numpy.random.default_rng(2).standard_normal((n, 3))
        X, h = oracle.solve(w, x0, 3, 1.0 / (2 * n))
        for r in results:
            assert numpy.array_equal(r[0][m], X) and numpy.array_equal(r[1][m], h)
    # degree_steps reached the ranks' own solvers: every map's step is its best-connected bin's
    import blueberry_amd as bb
    from tests._engines import OracleEngine
    for m in range(3):
        w = _oracle.wish_from_coords(_oracle.random_walk(sizes[m], seed=m))
        keep = numpy.triu(numpy.random.default_rng(m).random(w.shape) < 0.3, 1)
        keep |= numpy.triu(numpy.ones(w.shape, dtype=bool), 1) & ~numpy.triu(numpy.ones(w.shape, dtype=bool), 2)
        hm = numpy.where(keep | keep.T, w, 0.0)
        one = bb.StructureSolver(n_iter=3, dtype="float64", kind="wish", seed=2, engine=OracleEngine,
                                 distributed=False, degree_steps=True).fit(hm)
        for r in results:
            assert r[3][m] == one.lr_ == 1.0 / (2 * ((hm > 0).sum(axis=0).max() + 1))
            assert numpy.abs(r[4][m] / one.stress_ - 1).max() < 1e-12


# ---- select_exchange: the decision logic, with a scripted engine -----------------
class _ScriptedEngine(object):
    """Stands in for HipEngine: records what select_exchange does to it and lets a
    test script how each transport behaves (no GPU, no RCCL)."""

    def __init__(self, peer_ok=True, rccl_ok=True, peer_shift=0.0, peer_raises=False,
                 peer_sleep=0.0, rccl_sleep=0.0):
        self.world, self.rank = 1, 0
        self.x = numpy.arange(12.0).reshape(4, 3)
        self.calls = []
        self._comm_state = None
        self._comm_trial = None
        self.peer_ok, self.rccl_ok = peer_ok, rccl_ok
        self.peer_shift, self.peer_raises = peer_shift, peer_raises
        self.peer_sleep, self.rccl_sleep = peer_sleep, rccl_sleep
        self._peer_error = "scripted"

    def peer_setup(self):
        return self.peer_ok

    def comm_setup(self):
        return self.rccl_ok

    def get_coords(self):
        return self.x.copy()

    def set_coords(self, x):
        self.x = numpy.array(x, dtype=float)
        self.calls.append("set_coords")

    def sync(self):
        pass

    def peer_status(self):
        if self.peer_raises:
            raise RuntimeError("peer exchange: time limit")
        return 0

    def iterate_dist(self, k, lr):
        import time
        time.sleep(self.rccl_sleep * k)
        self.x = self.x - lr * k
        self.calls.append("rccl")

    def iterate_peer(self, k, lr):
        import time
        time.sleep(self.peer_sleep * k)
        self.x = self.x - lr * k * (1.0 + self.peer_shift)
        self.calls.append("peer")


class _ScriptedTorchEngine(_ScriptedEngine):
    """The same with the torch.distributed path played too (exchange_tensor / grad / apply):
    what the trial holds the peer exchange against when the library's communicator cannot
    be made."""

    def exchange_tensor(self):
        import torch
        return torch.zeros(3)

    def grad(self):
        import time
        time.sleep(self.rccl_sleep)

    def apply(self, lr):
        self.x = self.x - lr
        self.calls.append("torch")


@pytest.mark.parametrize("kwargs,expect", [
    (dict(peer_sleep=0.0, rccl_sleep=0.002), "peer"),          # agrees and is faster
    (dict(peer_sleep=0.002, rccl_sleep=0.0), "rccl"),          # agrees but is slower
    (dict(peer_shift=0.1, rccl_sleep=0.002), "rccl"),          # faster but WRONG
    (dict(peer_raises=True, rccl_sleep=0.002), "rccl"),        # a wait timed out
    (dict(peer_ok=False), "rccl"),                             # arenas could not be mapped
    (dict(peer_ok=False, rccl_ok=False), "torch"),             # neither
])
def test_select_exchange_auto_is_a_measured_validated_choice(one_rank_group, monkeypatch, kwargs,
                                                             expect):
    from blueberry_amd import solver
    monkeypatch.setattr(one_rank_group, "get_backend", lambda *a, **k: "nccl")
    e = _ScriptedEngine(**kwargs)
    x0 = e.get_coords()
    assert solver.select_exchange(e, 0.5, trial=True) == expect
    assert e._comm_state == expect
    assert numpy.array_equal(e.get_coords(), x0)               # the start is restored
    if kwargs.get("peer_ok", True) and kwargs.get("rccl_ok", True):
        agree = not kwargs.get("peer_shift") and not kwargs.get("peer_raises")
        assert e._comm_trial["agree"] == agree
    assert solver.select_exchange(e, 0.5) == expect            # decided once


@pytest.mark.parametrize("kwargs,expect", [
    (dict(rccl_ok=False, peer_sleep=0.0, rccl_sleep=0.002), "peer"),     # agrees with torch, faster
    (dict(rccl_ok=False, peer_shift=0.1, rccl_sleep=0.002), "torch"),    # faster but WRONG
    (dict(rccl_ok=False, peer_sleep=0.002, rccl_sleep=0.0), "torch"),    # agrees but slower
])
def test_trial_against_torch_when_the_library_communicator_cannot_be_made(one_rank_group,
                                                                           monkeypatch, kwargs, expect):
    """Round 3 gave the peer exchange up together with the library's RCCL communicator: without
    it there was no trial.  Now the peer exchange is held against torch.distributed's
    all-reduce instead, and the loser of THAT comparison is what runs."""
    from blueberry_amd import solver
    monkeypatch.setattr(one_rank_group, "get_backend", lambda *a, **k: "nccl")
    e = _ScriptedTorchEngine(**kwargs)
    x0 = e.get_coords()
    assert solver.select_exchange(e, 0.5, trial=True) == expect
    assert e._comm_trial["reference"] == "torch" and "torch" in e.calls and "rccl" not in e.calls
    assert numpy.array_equal(e.get_coords(), x0)               # the start was restored


def test_select_exchange_without_trial_is_rccl(one_rank_group, monkeypatch):
    """fit() never picks a transport by timing: auto = the library's RCCL communicator,
    torch.distributed if that cannot be made; BB_COMM_TRIAL=1 opts in to the trial."""
    from blueberry_amd import solver
    monkeypatch.setattr(one_rank_group, "get_backend", lambda *a, **k: "nccl")
    e = _ScriptedEngine(peer_sleep=0.0, rccl_sleep=0.002)
    assert solver.select_exchange(e, 0.5) == "rccl" and e.calls == []
    assert solver.select_exchange(_ScriptedEngine(rccl_ok=False), 0.5) == "torch"
    monkeypatch.setenv("BB_COMM_TRIAL", "1")
    assert solver.select_exchange(_ScriptedEngine(rccl_sleep=0.002), 0.5) == "peer"


def _trial_worker(rank, world, fail_rank, fail_leg):
    """One rank of a world-2 trial whose `fail_rank` raises at the start of `fail_leg`,
    BEFORE it joins that transport's collective -- the other rank is already inside.  Run
    with finish='exit': a collective nobody will ever complete may still be pending."""
    import torch.distributed as dist
    data = dist.new_group(backend="gloo")        # the transport's own communicator
    dist.get_backend = lambda *a, **k: "nccl"    # take select_exchange's RCCL branch
    from blueberry_amd import solver
    from tests._engines import ScriptedRankEngine
    e = ScriptedRankEngine(rank, world, data,
                           fail_leg=fail_leg if rank == fail_rank else None)
    x0 = e.get_coords()
    state = solver.select_exchange(e, 0.5, trial=True)
    return state, e._comm_trial, e.aborted, bool(numpy.array_equal(e.get_coords(), x0))


@pytest.mark.parametrize("fail_leg,expect,aborted", [("rccl", "torch", True),
                                                     ("peer", "rccl", False),
                                                     (None, "peer", False)])
def test_trial_with_a_rank_that_fails_before_its_collective(fail_leg, expect, aborted):
    """a rank whose warm-up raised used to skip the timed collective
    while the others entered it.  Now every stage ends with an agreement, waits on the
    device are bounded, and a communicator with a collective in flight is aborted: both
    ranks come out with the SAME transport, and nobody hangs."""
    results = run_ranks(_trial_worker, 2, 1, fail_leg, timeout=120, finish="exit",
                        env={"BB_TRIAL_SYNC_TIMEOUT_MS": "1500", "BB_COMM": None})
    assert [r[0] for r in results] == [expect, expect]
    for rank, (state, trial, was_aborted, restored) in enumerate(results):
        assert restored
        assert was_aborted == aborted
        assert trial["agree"] == (fail_leg is None)
        if fail_leg and rank == 1:                 # the rank that failed says why
            assert fail_leg in trial["error"]


NO_COMM_CHOICE = {"BB_COMM": None, "BB_COMM_TRIAL": None}


def _reuse_worker(rank, world):
    """Three 'fits' of one job: select_exchange on three fresh engines whose communicator
    cache is a dict that plays the library's (bb_comm_cached / _attach / _detach).  Before the
    third, rank 1 loses its cached communicator."""
    import torch.distributed as dist
    from blueberry_amd import solver
    from tests._engines import ScriptedRankEngine

    cache = {}                      # the library's process-wide cache, played

    class Engine(ScriptedRankEngine):
        setups = 0

        def comm_setup(self):
            Engine.setups += 1
            cache["comm"] = "made by fit %d" % Engine.setups
            self.comm = cache["comm"]
            return True

        def _comm_cached(self):
            return "comm" in cache

        def _comm_attach(self):
            self.comm = cache["comm"]
            return True

        def _comm_detach(self):
            self.comm = None

    # select_exchange must take its RCCL branch; the agreement (all_gather_object) runs
    # over the real gloo group
    dist.get_backend = lambda *a, **k: "nccl"
    out = []
    for fit in range(3):
        if fit == 2 and rank == 1:
            cache.clear()
        e = Engine(rank, world, None)
        state = solver.select_exchange(e, 0.5)
        out.append((state, Engine.setups, e.comm))
    return out


def test_two_fits_make_one_communicator():
    """every multi-rank fit() made a fresh RCCL communicator.  Now
    the first fit of a job makes it (comm_setup), later ones borrow it from the library's
    cache (solver.comm_reuse) -- and when one rank has lost its copy, EVERY rank makes a
    new one: the ranks agree before anybody attaches."""
    results = run_ranks(_reuse_worker, 2, timeout=120, env=NO_COMM_CHOICE)
    for rank in (0, 1):
        (s1, n1, c1), (s2, n2, c2), (s3, n3, c3) = results[rank]
        assert (s1, s2, s3) == ("rccl", "rccl", "rccl")
        assert (n1, n2) == (1, 1) and c2 == c1 == "made by fit 1"     # the second fit reused it
        assert n3 == 2 and c3 == "made by fit 2"                       # both ranks, not just rank 1


def _generation_worker(rank, world):
    """every rank answers 'cached and free', but the communicators are of
    DIFFERENT generations -- rank 0 replaced its stale entry while rank 1's earlier solver
    still held the old one.  Attaching them would hang the first all-reduce: comm_reuse
    compares the generations, nobody attaches, every rank makes a fresh one."""
    import torch.distributed as dist
    from blueberry_amd import solver
    from tests._engines import ScriptedRankEngine

    cache = {}
    attached = []

    class Engine(ScriptedRankEngine):
        setups = 0

        def comm_setup(self):
            Engine.setups += 1
            cache["comm"], cache["gen"] = "made by setup %d" % Engine.setups, 100 + Engine.setups
            self.comm = cache["comm"]
            return True

        def _comm_cached(self):
            return "comm" in cache

        def _comm_generation(self):
            return cache.get("gen", 0)

        def _comm_attach(self):
            attached.append(cache["gen"])
            self.comm = cache["comm"]
            return True

        def _comm_detach(self):
            self.comm = None

    dist.get_backend = lambda *a, **k: "nccl"
    out = []
    e = Engine(rank, world, None)
    out.append((solver.select_exchange(e, 0.5), Engine.setups, e.comm))     # fit 1: made
    e = Engine(rank, world, None)
    out.append((solver.select_exchange(e, 0.5), Engine.setups, e.comm))     # fit 2: reused
    if rank == 0:                     # rank 0 now holds a communicator of another generation
        cache["comm"], cache["gen"] = "someone else's", 7
    e = Engine(rank, world, None)
    out.append((solver.select_exchange(e, 0.5), Engine.setups, e.comm))     # fit 3: fresh
    return out, attached


def test_cached_communicators_of_different_generations_are_not_attached():
    results = run_ranks(_generation_worker, 2, timeout=120, env=NO_COMM_CHOICE)
    for rank in (0, 1):
        (s1, n1, c1), (s2, n2, c2), (s3, n3, c3) = results[rank][0]
        assert (s1, s2, s3) == ("rccl", "rccl", "rccl")
        assert (n1, n2) == (1, 1) and c2 == c1                     # same generation: reused
        assert n3 == 2 and c3 == "made by setup 2"                 # mismatch: fresh on BOTH ranks
        assert results[rank][1] == [101]                           # the only attach was fit 2's


def test_select_exchange_overrides(one_rank_group, monkeypatch):
    from blueberry_amd import solver
    monkeypatch.setattr(one_rank_group, "get_backend", lambda *a, **k: "nccl")
    for want, kwargs, expect in (("peer", {}, "peer"), ("rccl", {}, "rccl"),
                                 ("rccl", dict(rccl_ok=False), "torch"), ("torch", {}, "torch"),
                                 ("host", {}, "host")):
        monkeypatch.setenv("BB_COMM", want)
        e = _ScriptedEngine(**kwargs)
        assert solver.select_exchange(e, 0.5) == expect
        assert e.calls == []                                   # no trial when the choice is forced
    monkeypatch.setenv("BB_COMM", "peer")
    with pytest.raises(RuntimeError, match="could not be set up"):
        solver.select_exchange(_ScriptedEngine(peer_ok=False), 0.5)
    monkeypatch.setenv("BB_COMM", "bogus")
    with pytest.raises(ValueError):
        solver.select_exchange(_ScriptedEngine(), 0.5)


def test_select_exchange_on_gloo_is_host_staged(one_rank_group):
    from blueberry_amd import solver
    e = _ScriptedEngine()
    assert solver.select_exchange(e, 0.5) == "host" and e.calls == []
