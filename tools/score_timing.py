"""Kernel times of bb_solver_score (SPEC 2.8) with the units resident: N = 24,926
fp32 dense, N = 4,097 fp64 and BASELINE config 5 (blocked-sparse genome at 10 kb, fp32).  The
wish is generated on the device (bb_solver_set_wish_from_coords).  HIP events around each of
the call's three kernels (bb_solver_set_timing + bb_solver_get_score_timing); one warm call,
then the median (min..max) of `--reps` calls.  For the profile kernel the unit bytes / time is
put beside 8 TB/s; for scale, one solver iteration at the same size (event-timed sweep + reduce,
the median of `--reps` blocks of `--steps`)."""
import argparse
import os
import sys

import numpy

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from blueberry_amd.solver import HipEngine, tiles_from_blocks  # noqa: E402
from blueberry_amd.utils import genome_boundaries  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=11)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--cases", default="25k,4097,config5")
a = ap.parse_args()

CASES = {"25k": (24926, "float32", False), "4097": (4097, "float64", False),
         "config5": (309568, "float32", True)}
HBM_BYTES_PER_MS = 8e12 / 1e3

for name in a.cases.split(","):
    n, dtype, genome = CASES[name]
    tiles, pairs = None, n * (n - 1) // 2
    if genome:
        tiles, pairs = tiles_from_blocks(n, genome_boundaries(n), 1000, dtype)
    xs = numpy.cumsum(numpy.random.default_rng(0).standard_normal((n, 3)), axis=0)
    x0 = xs + 0.5 * numpy.random.default_rng(1).standard_normal(xs.shape)
    eng = HipEngine(n, dtype, tiles=tiles)
    eng.set_wish_from_coords(xs)
    unit_bytes = eng.traffic()["unit_bytes"]
    eng.set_coords(x0)
    eng.set_timing(1)
    eng.score(x0)                                         # warm
    t = []
    for _ in range(a.reps):
        profile, bins = eng.score(x0)
        t.append(eng.score_timing())
    t = numpy.array(t)
    step = []
    for _ in range(a.reps):
        eng.set_timing(1)
        eng.iterate(a.steps, 0.5 / n)
        eng.sync()
        tm = eng.timing()
        step.append(tm["grad_ms"] + tm["reduce_ms"])
    path = eng.iteration_path()[0]
    eng.close()
    med, lo, hi = numpy.median(t, axis=0), t.min(axis=0), t.max(axis=0)
    assert int(profile[:, 0].sum()) > 0 and bins[:, 0].sum() == 2 * profile[:, 0].sum()
    print("%-8s N=%-7d %s: %d constrained pairs of %d stored, %.1f MB of units" % (
        name, n, dtype, int(profile[:, 0].sum()), pairs, unit_bytes / 1e6), flush=True)
    for k, kernel in enumerate(("profile", "fold", "per bin")):
        print("    %-8s %9.4f ms (min %.4f max %.4f, %d calls)" % (kernel, med[k], lo[k], hi[k], t.shape[0]),
              flush=True)
    print("    profile kernel: %.1f GB/s of units = %.3f of 8 TB/s; %.2f Gpairs/s" % (
        unit_bytes / med[0] / 1e6, unit_bytes / med[0] / HBM_BYTES_PER_MS, pairs / med[0] / 1e6), flush=True)
    print("    one solver iteration (%s): %.4f ms (median of %d blocks of %d; sweep + reduce by events)" % (
        path, float(numpy.median(step)), len(step), a.steps), flush=True)
