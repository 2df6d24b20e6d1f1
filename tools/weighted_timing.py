"""ms/step and Gpair-updates/s of the weighted stress (SPEC 2.3.1), q = 0, 1, 2, for
DESIGN.md 4.13: N = 50,000 dense fp32, N = 24,926 fp32, N = 963 fp64 (row-owner path) and
BASELINE config 5 (blocked-sparse genome at 10 kb, fp32).  The wish is generated on the
device (delta_ij = |x*_i - x*_j|, bb_solver_set_wish_from_coords).  Each case times
`--reps` blocks of `--steps` iterations after a settle block and reports the median and
the spread (min..max) of the blocks; the three weight powers are interleaved block by block
so that clock drift falls on all of them alike."""
import argparse
import os
import sys
import time

import numpy

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from blueberry_amd.solver import HipEngine, tiles_from_blocks  # noqa: E402
from blueberry_amd.utils import genome_boundaries  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--cases", default="50k,25k,963,config5")
a = ap.parse_args()

CASES = {"50k": (50000, "float32", False), "25k": (24926, "float32", False),
         "963": (963, "float64", False), "config5": (309568, "float32", True)}

for name in a.cases.split(","):
    n, dtype, genome = CASES[name]
    tiles, pairs = None, n * (n - 1) // 2
    if genome:
        tiles, pairs = tiles_from_blocks(n, genome_boundaries(n), 1000, dtype)
    xs = numpy.cumsum(numpy.random.default_rng(0).standard_normal((n, 3)), axis=0)
    x0 = xs + 0.5 * numpy.random.default_rng(1).standard_normal(xs.shape)
    eng = HipEngine(n, dtype, tiles=tiles)
    eng.set_wish_from_coords(xs)
    lrs = {}
    for q in (0, 1, 2):
        eng.set_weight_power(q)
        lrs[q] = 1.0 / (2.0 * eng.weight_sums().max())
    times = {0: [], 1: [], 2: []}
    for rep in range(a.reps + 1):
        for q in (0, 1, 2):
            eng.set_weight_power(q)
            eng.set_coords(x0)
            eng.sync()
            t0 = time.perf_counter()
            eng.iterate(a.steps, lrs[q])
            eng.sync()
            dt = (time.perf_counter() - t0) * 1e3 / a.steps
            if rep > 0:                                  # the first block settles the clocks
                times[q].append(dt)
    path = eng.iteration_path()[0]
    eng.close()
    base = numpy.median(times[0])
    for q in (0, 1, 2):
        t = numpy.array(times[q])
        med = float(numpy.median(t))
        print("%-8s N=%-7d %s %-9s q=%d: %.4f ms/step (min %.4f max %.4f, %d blocks of %d) "
              "%.1f Gpair-updates/s  ratio to q=0 %.3f"
              % (name, n, dtype, path, q, med, t.min(), t.max(), t.size, a.steps,
                 pairs / med / 1e6, med / base), flush=True)
