"""GPU: StructureSolver(devices=[...]) -- several solvers of ONE process, a host thread each,
their partials summed by group_apply_kernel behind HIP events (bb_group_*).

The test box has one GPU, so every group here repeats device 0 (the rehearsal form): members
take turns on the chip.  What is checked is what does not depend on the number of chips: the
sums are those of the process-per-rank peer exchange (two-launch form) at the same world size,
bit for bit; every member holds the same bits; every input form and option reaches the
members; the oracle holds at chr1@10kb size."""
import ctypes
import os
import subprocess
import sys

import numpy
import pytest

from tests._ranks import no_rank_process_outlives_its_test         # noqa: F401 -- autouse
from tests._util import host_threads as _host_threads
from tests._util import rel as _rel

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _incomplete_wish(n):
    """Wish distances of a random walk with a third of the pairs absent (delta = 0), so that
    degree_steps gives every bin a step of its own.  Module level: rank processes call it."""
    from tests import _oracle
    w = _oracle.wish_from_coords(_oracle.random_walk(n))
    drop = numpy.triu(numpy.random.default_rng(5).random((n, n)) < 0.33, 1)
    w[drop | drop.T] = 0.0
    return w


def _set_wish(eng, make, n):
    eng.set_wish_dense(make(n), "wish", 3.0)


# ---- 1. bit for bit the process-per-rank peer exchange -----------------------------------

def _peer_run(world, n, dtype, x0, mu, degree_steps, tol, check_every, k):
    """The two-launch peer exchange, a process per rank (tests/_ranks.py), driven the way
    StructureSolver drives one rank: returns rank 0's coordinates and stress history and
    whether all ranks agree."""
    from blueberry_amd.solver import degree_step_factors
    from tests import _ranks
    ranks = _ranks.peer_ranks(world, n, dtype)
    assert all(r.peer_form() == "two launches" for r in ranks)
    lr = 1.0 / (2 * n)
    for r in ranks:
        r.run(_set_wish, _incomplete_wish, n)
    if degree_steps:
        deg = ranks[0].degrees()
        for r in ranks[1:]:
            deg = deg + r.degrees()
        lr, scale = degree_step_factors(deg)
        for r in ranks:
            r.set_bin_steps(scale)
    for r in ranks:
        r.set_coords(x0)
        r.set_momentum(mu)
    done = 0
    while done < k:
        step = k - done if tol is None else min(check_every, k - done)
        for _ in range(step):                       # one thread feeds them: step by step
            for r in ranks:
                r.iterate_peer(1, lr)
        done += step
        if tol is not None:
            h = ranks[0].stress_history()
            if h.size >= 2 and h[-2] > 0 and abs(h[-2] - h[-1]) <= tol * h[-2]:
                break
    out = []
    for r in ranks:
        assert r.peer_status() == 0
        out.append((r.get_coords(), r.stress_history()))
        r.close()
    same = all(numpy.array_equal(X, out[0][0]) and numpy.array_equal(h, out[0][1])
               for X, h in out[1:])
    return out[0][0], out[0][1], same


@pytest.mark.parametrize("mode", ["plain", "momentum", "degree_steps", "tol"])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("world", [2, 3])
def test_group_equals_process_per_rank_bit_for_bit(world, dtype, mode, monkeypatch):
    monkeypatch.setenv("BB_PEER_FUSED", "0")
    monkeypatch.setenv("BB_PEER_TIMEOUT_MS", "20000")
    import blueberry_amd as bb
    n, k = 3000, 12
    mu = 0.5 if mode == "momentum" else 0.0
    tol = 1e-2 if mode == "tol" else None          # this map's decrease dips below 1 % near step 9
    ds = mode == "degree_steps"
    x0 = numpy.random.default_rng(4).standard_normal((n, 3)) * 50.0
    X_p, h_p, same = _peer_run(world, n, dtype, x0, mu, ds, tol, 1, 60 if tol else k)
    assert same
    s = bb.StructureSolver(n_iter=60 if tol else k, dtype=dtype, kind="wish", momentum=mu,
                           degree_steps=ds, tol=tol, check_every=1, devices=[0] * world)
    s.fit(_incomplete_wish(n), init=x0)
    assert s.exchange_ == "group" and s.devices_ == [0] * world
    assert numpy.array_equal(s.structure_, X_p), _rel(s.structure_, X_p)
    assert numpy.array_equal(s.stress_, h_p)
    assert s.n_iter_ == h_p.size
    if tol is not None:
        assert s.n_iter_ < 60                        # the stopping rule did stop it


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_group_members_hold_identical_bits(dtype):
    """Every member sums the same vectors in the same order: identical coordinates, velocity
    effects and stress histories, across two iterate calls (the events carry over)."""
    from blueberry_amd.solver import GroupEngine, degree_step_factors
    n = 2600
    w = _incomplete_wish(n)
    x0 = numpy.random.default_rng(6).standard_normal((n, 3)) * 50.0
    g = GroupEngine(n, dtype, [0, 0, 0])
    try:
        g.set_wish_dense(w, "wish", 3.0)
        lr, scale = degree_step_factors(g.degrees())
        g.set_bin_steps(scale)
        g.set_coords(x0)
        g.set_momentum(0.3)
        g.iterate(4, lr)
        g.iterate(3, lr)
        Xs, hs = g.member_coords(), g.member_stress_histories()
    finally:
        g.close()
    assert hs[0].size == 7
    for X, h in zip(Xs[1:], hs[1:]):
        assert numpy.array_equal(X, Xs[0]) and numpy.array_equal(h, hs[0])


# ---- 2. the oracle at chr1@10kb size ------------------------------------------------------

@pytest.fixture(scope="module")
def chr1_reference():
    from tests import _oracle
    n, k = 24926, 20
    xs = _oracle.random_walk(n)
    x0 = _oracle.noisy_init(xs)
    X_ref, h_ref = _oracle.solve_gen_mt(xs, x0, k, 1.0 / (2 * n), _host_threads(), f64=False)
    return xs, x0, X_ref, h_ref


@pytest.mark.parametrize("world", [2, 3, 8])
def test_group_fp32_chr1_10kb_sized_vs_oracle(chr1_reference, world):
    from blueberry_amd.solver import GroupEngine
    xs, x0, X_ref, h_ref = chr1_reference
    n, k = xs.shape[0], h_ref.shape[0]
    g = GroupEngine(n, "float32", [0] * world)
    try:
        g.set_wish_from_coords(xs)
        g.set_coords(x0)
        g.iterate(k, 1.0 / (2 * n))
        Xs, hs = g.member_coords(), g.member_stress_histories()
    finally:
        g.close()
    err_s, err_x = float(numpy.abs(hs[0] / h_ref - 1).max()), _rel(Xs[0], X_ref)
    print("N=%d K=%d fp32, %d members vs oracle: stress %.2e coords %.2e" % (n, k, world, err_s, err_x))
    assert err_s < 1e-5 and err_x < 1e-5, (err_s, err_x)
    assert all(numpy.array_equal(X, Xs[0]) for X in Xs[1:])


def test_group_fp64_vs_oracle(oracle):
    import blueberry_amd as bb
    from tests import _oracle
    n, k = 963, 15
    xs = _oracle.random_walk(n)
    w = _oracle.wish_from_coords(xs)
    x0 = _oracle.noisy_init(xs)
    X_ref, h_ref = oracle.solve(w, x0, k, 1.0 / (2 * n))
    s = bb.StructureSolver(n_iter=k, dtype="float64", kind="wish", devices=[0, 0, 0]).fit(w, init=x0)
    assert numpy.abs(s.stress_ / h_ref - 1).max() < 1e-12
    assert _rel(s.structure_, X_ref) < 1e-12


# ---- 3. every input form ------------------------------------------------------------------

TOLS = [("float64", 1e-12), ("float32", 1e-5)]


def _agree(a, b, tol):
    assert numpy.abs(a.stress_ / b.stress_ - 1).max() < tol
    assert _rel(a.structure_, b.structure_) < tol


@pytest.mark.parametrize("dtype,tol", TOLS)
def test_group_blocked_sparse_input(dtype, tol):
    import scipy.sparse
    import blueberry_amd as bb
    from tests import _oracle
    n, k = 3000, 8
    w = _oracle.wish_from_coords(_oracle.random_walk(n))
    rng = numpy.random.default_rng(2)
    i = rng.integers(0, n, 150000)
    j = numpy.clip(i + rng.integers(-700, 700, i.size), 0, n - 1)   # a band: tiles are missing
    sp = scipy.sparse.coo_matrix((w[i, j], (i, j)), shape=(n, n))
    x0 = numpy.random.default_rng(3).standard_normal((n, 3))
    one = bb.StructureSolver(n_iter=k, dtype=dtype, kind="wish", degree_steps=True).fit(sp, init=x0)
    grp = bb.StructureSolver(n_iter=k, dtype=dtype, kind="wish", degree_steps=True,
                             devices=[0, 0, 0]).fit(sp, init=x0)
    _agree(grp, one, tol)


def _triples_case():
    rng = numpy.random.default_rng(8)
    n_bins, res = 700, 10000
    bi = rng.integers(0, n_bins, 40000)
    bj = numpy.minimum(n_bins - 1, bi + rng.geometric(0.02, 40000))
    key = numpy.unique(bi * n_bins + bj)
    bi, bj = key // n_bins, key % n_bins
    counts = rng.integers(1, 400, bi.size).astype(float)
    triples = numpy.stack([bi * float(res), bj * float(res), counts], 1)
    kr = 0.5 + rng.random(n_bins)
    kr[rng.random(n_bins) < 0.05] = numpy.nan
    ke = 40.0 / (1.0 + numpy.arange(n_bins)) + 0.2
    return triples, res, n_bins, kr, ke


@pytest.mark.parametrize("dtype,tol", TOLS)
def test_group_fit_triples_with_kr(dtype, tol):
    import blueberry_amd as bb
    triples, res, n_bins, kr, ke = _triples_case()
    x0 = numpy.random.default_rng(1).standard_normal((n_bins + 1, 3))
    one = bb.StructureSolver(n_iter=6, dtype=dtype).fit_triples(
        triples, res, n_bins, KRnorm=kr, KRexpected=ke, init=x0)
    grp = bb.StructureSolver(n_iter=6, dtype=dtype, devices=[0, 0, 0]).fit_triples(
        triples, res, n_bins, KRnorm=kr, KRexpected=ke, init=x0)
    _agree(grp, one, tol)


@pytest.mark.parametrize("dtype,tol", TOLS)
def test_group_resident_contactmap_is_not_downloaded(dtype, tol, monkeypatch):
    import blueberry_amd as bb
    triples, res, n_bins, kr, ke = _triples_case()
    x0 = numpy.random.default_rng(1).standard_normal((n_bins + 1, 3))

    def make():
        cm = bb.ContactMap.from_matrix(bb.datatypes.scatter_triples(triples, res, n_bins),
                                       resolution=res, KRnorm=kr, KRexpected=ke)
        cm.normalize()
        assert cm.is_resident
        return cm
    one = bb.StructureSolver(n_iter=6, dtype=dtype).fit(make(), init=x0)
    cm = make()
    downloads = []
    real = bb.datatypes._DeviceMatrix.to_host
    monkeypatch.setattr(bb.datatypes._DeviceMatrix, "to_host",
                        lambda self: downloads.append(1) or real(self))
    grp = bb.StructureSolver(n_iter=6, dtype=dtype, devices=[0, 0, 0]).fit(cm, init=x0)
    assert downloads == [] and cm.is_resident
    _agree(grp, one, tol)


# ---- 4. weighting and the spectral start ---------------------------------------------------

@pytest.mark.parametrize("q", [1, 2])
@pytest.mark.parametrize("dtype,tol", TOLS)
def test_group_weighted_stress(dtype, tol, q):
    import blueberry_amd as bb
    n = 2500
    w = _incomplete_wish(n)
    x0 = numpy.random.default_rng(3).standard_normal((n, 3)) * 50.0
    kw = dict(n_iter=8, dtype=dtype, kind="wish", weight_power=q, degree_steps=True)
    one = bb.StructureSolver(**kw).fit(w, init=x0)
    grp = bb.StructureSolver(devices=[0, 0, 0], **kw).fit(w, init=x0)
    _agree(grp, one, tol)


@pytest.mark.parametrize("dtype,tol", [("float64", 1e-9), ("float32", 1e-3)])
def test_group_spectral_start(dtype, tol):
    import blueberry_amd as bb
    from tests import _oracle
    n = 900
    w = _oracle.wish_from_coords(_oracle.random_walk(n))
    kw = dict(n_iter=0, dtype=dtype, kind="wish", init="spectral", spectral_tol=0.0)
    one = bb.StructureSolver(**kw).fit(w)
    grp = bb.StructureSolver(devices=[0, 0, 0], **kw).fit(w)
    d_one, d_grp = _oracle.wish_from_coords(one.structure_), _oracle.wish_from_coords(grp.structure_)
    assert numpy.abs(d_grp - d_one).max() < tol * w.max()
    assert numpy.abs(grp.structure_ - one.structure_).max() < 10 * tol * w.max()


# ---- 5. validation ---------------------------------------------------------------------------

def test_group_device_index_out_of_range():
    import blueberry_amd as bb
    count = ctypes.c_int()
    bb._lib.check(bb._lib.load().bb_device_count(count), "bb_device_count")
    with pytest.raises(ValueError, match="out of range"):
        bb.StructureSolver(n_iter=1, devices=[0, count.value]).fit(numpy.ones((50, 50)))
    with pytest.raises(ValueError, match="out of range"):
        bb.StructureSolver(n_iter=1, devices=[count.value]).fit(numpy.ones((50, 50)))
    one = bb.StructureSolver(n_iter=2, kind="wish", devices=[0]).fit(numpy.ones((50, 50)))
    assert one.devices_ == [0] and one.exchange_ is None and one.stress_.size == 2


def test_group_create_and_iterate_errors():
    from blueberry_amd import _lib
    from blueberry_amd.solver import HipEngine
    lib = _lib.load()

    def create(engs):
        g = ctypes.c_void_p()
        arr = (ctypes.c_void_p * len(engs))(*[e._h.value for e in engs])
        rc = lib.bb_group_create(g, arr, len(engs))
        return rc, g, _lib.last_error()

    a = [HipEngine(600, "float32", rank=r, world=2) for r in range(2)]
    try:
        rc, _, msg = create([a[1], a[0]])                        # rank order
        assert rc == _lib.BB_ERR_INVALID and "rank" in msg, msg
        rc, _, msg = create([a[0]])                               # world 2 in a group of 1
        assert rc == _lib.BB_ERR_INVALID and "world" in msg, msg
        b = HipEngine(700, "float32", rank=1, world=2)
        rc, _, msg = create([a[0], b])                            # n_bins
        b.close()
        assert rc == _lib.BB_ERR_INVALID and "n_bins" in msg, msg
        c = HipEngine(600, "float64", rank=1, world=2)
        rc, _, msg = create([a[0], c])                            # dtype
        c.close()
        assert rc == _lib.BB_ERR_INVALID and "dtype" in msg, msg
        rc, g, msg = create(a)
        assert rc == _lib.BB_OK, msg
        try:
            rc = lib.bb_group_iterate(g, 1, 1e-3)                 # no wish distances yet
            assert rc == _lib.BB_ERR_STATE
            w = numpy.random.default_rng(0).random((600, 600)) + 1.0
            for e in a:
                e.set_wish_dense(w + w.T, "wish", 3.0)
                e.set_coords(numpy.random.default_rng(1).standard_normal((600, 3)))
            rc = lib.bb_group_iterate(g, (1 << 20) + 1, 1e-3)     # past the history capacity
            assert rc == _lib.BB_ERR_STATE and "history" in _lib.last_error()
            assert a[0].stress_history().size == 0                # nothing was enqueued
            assert lib.bb_group_iterate(g, 2, 1e-3) == _lib.BB_OK
            assert a[0].stress_history().size == 2
        finally:
            lib.bb_group_destroy(g)
    finally:
        for e in a:
            e.close()


def test_group_fit_many_is_refused():
    import blueberry_amd as bb
    with pytest.raises(ValueError, match="fit_many"):
        bb.StructureSolver(n_iter=1, devices=[0, 0]).fit_many([numpy.ones((10, 10))])


# ---- 6. no torch on this path ----------------------------------------------------------------

def test_group_fit_does_not_import_torch():
    code = (
        "import sys, numpy\n"
        "sys.path.insert(0, %r)\n"
        "import blueberry_amd as bb\n"
        "from tests import _oracle\n"
        "xs = _oracle.random_walk(800)\n"
        "s = bb.StructureSolver(n_iter=5, kind='wish', devices=[0, 0]).fit(\n"
        "    _oracle.wish_from_coords(xs), init=_oracle.noisy_init(xs))\n"
        "assert s.exchange_ == 'group' and s.stress_.size == 5\n"
        "assert 'torch' not in sys.modules, 'torch was imported'\n"
        "print('ok')\n" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
