"""ms per iteration of StructureSolver(devices=[0] * R): R members of one process, a host
thread each, the exchange ordered by HIP events (bb_group_*), for R = 1, 2, 3, 8 at
N = 24,926 and N = 50,000 dense fp32 (wish generated on the device from x*,
bb_solver_set_wish_from_coords).  R = 1 is the one-device path (devices=[0] is device=0).

On ONE GPU the members take turns on the chip: each sweeps 1/R of the units, so the sweeps
add up to one device's sweep, and what R > 1 adds on top is the cost of the host threads,
barriers, event waits and the extra reduce and group_apply_kernel launches.  These figures do
NOT show scaling over several GPUs, and nothing here measures the per-iteration gather over
xGMI.  Each case times `--reps` blocks of `--steps` iterations after a settle block (median
and min..max of the blocks).

    python tools/group_timing.py [--sizes 24926,50000] [--worlds 1,2,3,8] [--steps 50] [--reps 5]"""
import argparse
import os
import sys
import time

import numpy

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from blueberry_amd.solver import GroupEngine, HipEngine  # noqa: E402
from tests import _oracle  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="24926,50000")
ap.add_argument("--worlds", default="1,2,3,8")
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--reps", type=int, default=5)
a = ap.parse_args()

print("devices=[0]*R on one MI355X, dense fp32: members take turns on one chip -- host threads "
      "and event waits, not scaling")
print("%8s %3s %10s %20s" % ("N", "R", "ms/iter", "min..max of blocks"))
for n in [int(v) for v in a.sizes.split(",")]:
    xs = _oracle.random_walk(n)
    x0 = _oracle.noisy_init(xs)
    lr = 1.0 / (2 * n)
    for R in [int(v) for v in a.worlds.split(",")]:
        eng = HipEngine(n, "float32") if R == 1 else GroupEngine(n, "float32", [0] * R)
        try:
            eng.set_wish_from_coords(xs)
            eng.set_coords(x0)
            eng.iterate(a.steps, lr)                    # settle
            eng.sync()
            ms = []
            for _ in range(a.reps):
                eng.set_coords(x0)                      # (resets the stress history)
                eng.sync()
                t0 = time.perf_counter()
                eng.iterate(a.steps, lr)
                eng.sync()
                ms.append((time.perf_counter() - t0) * 1e3 / a.steps)
            assert numpy.isfinite(eng.stress_history()).all()
        finally:
            eng.close()
        print("%8d %3d %10.3f %9.3f..%-9.3f" % (n, R, float(numpy.median(ms)), min(ms), max(ms)),
              flush=True)
