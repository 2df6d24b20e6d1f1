"""GPU: the stage times the calls report by HIP events -- the `ms` of bb_structures_compare,
`score_timing()`, bb_cm_coarsen_timing, bb_triples_coarsen_timing, bb_sig_timing,
`GeodesicRows.timing()`, and the sort / scan times of bb_sig_q_values -- on a 130-bin map.

A time is checked for what can be known of it: finite, positive where a kernel ran, exactly 0 for a
stage the call skipped; and asking for the times changes nothing else the call returns."""
import functools

import numpy
import pytest

import blueberry_amd as bb
from blueberry_amd import _lib
from blueberry_amd import fithic as fh
from tests import _balance_model as bm
from tests import _compare_model as cmodel
from tests import _fithic_model as fm
from tests import _score_model as smodel
from tests import _triples_model as tm
from tests.test_gpu_compare import _compare

pytestmark = pytest.mark.gpu

N = 130
RES = 10000


@functools.lru_cache(maxsize=None)
def _raw():
    """(the raw (N + 1)^2 map, its upper triangle as triples): made once, never changed."""
    m = bm.hic_like_raw(N + 1)
    t = tm.triples_of_matrix(m, RES, border=False)
    t.setflags(write=False)
    return m, t


def _significance(X):
    """The listed cells of the raw map on handle X over every diagonal from 1, and the number of tests."""
    m = _raw()[0]
    ks = fm.in_range(N, RES, 0, N * RES)
    possible, observed = fm.tallies(m, N, ks)
    n_reads = float(observed.sum())
    res = fh.significance_list(X, N, ks[0], ks[-1], numpy.ones(N), None, fm.decay_prior(N, n_reads), n_reads)
    return res, int(sum(possible[k] for k in ks))


def _positive(*times):
    return all(numpy.isfinite(t) and t > 0.0 for t in times)


@pytest.mark.parametrize("ranks", [False, True])
def test_compare_stage_times(ranks):
    A, B = cmodel.float_case(N)
    plain = _compare(A, B, None, cmodel.IDENTITY13, ranks=ranks)
    timed = _compare(A, B, None, cmodel.IDENTITY13, ranks=ranks, want_ms=True)
    ms = timed[5]
    print("compare, ranks = %s: ms = %s" % (ranks, ms))
    assert numpy.isfinite(ms).all() and (ms >= 0.0).all()
    assert (ms[:4] > 0.0).all()                        # transform, pairs, fold, bins
    assert ms[4] > 0.0 if ranks else ms[4] == 0.0
    for got, want in zip(timed[:5], plain):
        assert (got is None and want is None) or got.tobytes() == want.tobytes()


def test_score_stage_times():
    from blueberry_amd.solver import HipEngine
    w, x = smodel.float_case(N)
    eng = HipEngine(N, "float32")
    try:
        eng.set_wish_dense(w, "wish", 3.0)
        eng.set_timing(True)
        eng.score(x)
        t = eng.score_timing()
        print("score: ms = %s" % (t,))
        assert len(t) == 3 and _positive(*t)
        eng.loglog(x)
        t = eng.score_timing()
        print("loglog: ms = %s" % (t,))
        assert _positive(t[0], t[1]) and t[2] == 0.0     # no per-bin kernel ran
    finally:
        eng.close()


def test_dense_coarsen_time():
    cm = bb.ContactMap.from_matrix(_raw()[0], resolution=RES)
    ms = cm.coarsen(2)._dev._get(_lib.c_dbl, "coarsen_timing")
    print("bb_cm_coarsen_timing: %r" % ms)
    assert _positive(ms)


def test_triples_coarsen_time():
    with bb.DeviceTriples(_raw()[1], RES, 0) as dev, dev.coarsen(N, 2) as pooled:
        ms = pooled._get(_lib.c_dbl, "coarsen_timing")
        print("bb_triples_coarsen_timing: %r (%d pooled cells)" % (ms, pooled.n))
        assert pooled.n > 0 and _positive(ms)
    # no triple: the count kernel runs over the 65 coarse rows, nothing is written
    with bb.DeviceTriples(numpy.zeros((0, 3)), RES, 0) as dev, dev.coarsen(N, 2) as pooled:
        ms = pooled._get(_lib.c_dbl, "coarsen_timing")
        print("bb_triples_coarsen_timing, no triple: %r" % ms)
        assert pooled.n == 0 and numpy.isfinite(ms) and ms >= 0.0


def test_significance_times():
    cm = bb.ContactMap.from_matrix(_raw()[0], resolution=RES)
    res = _significance(cm)[0]
    try:
        list_ms, p_ms = res.timing()
        print("bb_sig_timing: list %r, p %r (%d cells)" % (list_ms, p_ms, res.size()[0]))
        assert res.size()[0] > 0 and _positive(list_ms, p_ms)
    finally:
        res.close()


def test_shortest_paths_times():
    with bb.DeviceTriples(_raw()[1], RES, 0) as dev, dev.shortest_paths(N, [0, N // 2]) as rows:
        weights_ms, sweeps_ms = rows.timing()
        print("GeodesicRows.timing: weights %r, sweeps %r" % (weights_ms, sweeps_ms))
        assert _positive(weights_ms, sweeps_ms)


def test_q_values_are_the_same_timed_or_not():
    cm = bb.ContactMap.from_matrix(_raw()[0], resolution=RES)
    res, n_tests = _significance(cm)
    try:
        res._call("q_values", n_tests, None, None)         # sort_ms = scan_ms = NULL
        untimed = res.read_q()
        sort_ms, scan_ms = res.q_values(n_tests)
        print("bb_sig_q_values: sort %r, scan %r" % (sort_ms, scan_ms))
        assert untimed.shape[0] > 0 and _positive(sort_ms, scan_ms)
        assert res.read_q().tobytes() == untimed.tobytes()
    finally:
        res.close()
