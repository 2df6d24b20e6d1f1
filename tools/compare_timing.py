"""Kernel times of bb_structures_compare (SPEC 2.10): a random walk of N bins
against a noisy, rotated copy, at N = 24,926 without ranks and N = 8,192 with ranks.  HIP events
around the transform, the pair pass, its fold, the per-bin pass and the ranks (the entry's `ms`);
one warm call, then the median (min..max) of `--reps` calls, and the wall time of the whole
Python call (uploads, both device calls, the SVD, read-back) beside them.  The pair pass is put
beside its own pair count only: no peak rate is quoted."""
import argparse
import os
import sys
import time

import numpy

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import blueberry_amd as bb  # noqa: E402
from blueberry_amd import _lib  # noqa: E402
from blueberry_amd.compare import superposition  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--cases", default="24926,8192r")
a = ap.parse_args()

CASES = {"24926": (24926, False), "8192r": (8192, True), "2049r": (2049, True), "4097": (4097, False)}
P = _lib.as_f64_ptr
lib = _lib.load()

for name in a.cases.split(","):
    n, ranks = CASES[name]
    A = numpy.cumsum(numpy.random.default_rng(0).standard_normal((n, 3)), axis=0)
    q, _ = numpy.linalg.qr(numpy.random.default_rng(2).standard_normal((3, 3)))
    B = (A + 0.5 * numpy.random.default_rng(1).standard_normal(A.shape)) @ q.T + 3.0
    moments = numpy.zeros(18)
    _lib.check(lib.bb_structures_moments(P(A), P(B), None, n, 0, P(moments)), "bb_structures_moments")
    R, t, s, _ = superposition(moments)
    tr = numpy.concatenate([R.reshape(9), t, [s]])
    dev, profile, bins = numpy.zeros(n), numpy.zeros((n, 7)), numpy.zeros((n, 2))
    rank_sums, ms = numpy.zeros(4), numpy.zeros(5)
    times = []
    for rep in range(a.reps + 1):                         # (the first call is the warm one)
        _lib.check(lib.bb_structures_compare(P(A), P(B), None, n, P(tr), _lib.BB_CMP_SPEARMAN if ranks else 0, 0,
                                             None, P(dev), P(profile), P(bins), P(rank_sums) if ranks else None,
                                             P(ms)), "bb_structures_compare")
        if rep:
            times.append(ms.copy())
    times = numpy.array(times)
    pairs = n * (n - 1) // 2
    assert int(profile[:, 0].sum()) == pairs and bins[:, 0].sum() == 2 * pairs
    t0 = time.perf_counter()
    rep = bb.compare_structures(A, B, spearman=ranks)
    wall = (time.perf_counter() - t0) * 1e3
    med, lo, hi = numpy.median(times, axis=0), times.min(axis=0), times.max(axis=0)
    print("N=%-6d %s: %d pairs; rmsd %.4f, distance rmsd %.4f, pearson %.6f, spearman %.6f" % (
        n, "with ranks" if ranks else "no ranks", pairs, rep.rmsd, rep.distance_rmsd, rep.distance_pearson,
        rep.distance_spearman), flush=True)
    for k, kernel in enumerate(("transform", "pairs", "fold", "per bin", "ranks")):
        if kernel != "ranks" or ranks:
            print("    %-9s %10.4f ms (min %.4f max %.4f, %d calls)" % (kernel, med[k], lo[k], hi[k], times.shape[0]),
                  flush=True)
    print("    pair pass: %.2f Gpairs/s; per-bin pass: %.2f Gpairs/s (every pair twice)" % (
        pairs / med[1] / 1e6, 2 * pairs / med[3] / 1e6), flush=True)
    if ranks:
        print("    ranks: %.1f Mpairs/s over two sorts of %d keys, %.1f MB of rank buffers" % (
            pairs / med[4] / 1e3, pairs, 40.0 * pairs / 1e6), flush=True)
    print("    compare_structures, host to host: %.1f ms" % wall, flush=True)
