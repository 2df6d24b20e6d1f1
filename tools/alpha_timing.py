"""Times of alpha='auto' (SPEC 2.11) at N = 24,926 fp32 from a resident ContactMap
of counts c = D^-3.4 of a random walk:
  * bb_solver_loglog's profile and fold kernels next to bb_solver_score's on the same units (HIP
    events, bb_solver_set_timing + bb_solver_get_score_timing), unit bytes / time beside 8 TB/s;
  * bb_solver_repower (wall time of the call: the pow kernel, the sync and, below the row-owner
    limit, the rebuilt matrix) next to a read-write stream of as many bytes (a device-to-device
    copy, HIP events);
  * a whole alpha='auto' fit next to one fixed-alpha fit at the same n_iter (wall time, the map
    resident before both).  A float alpha takes the code path it took before 'auto' existed.
One warm call each, then the median (min..max) of `--reps`."""
import argparse
import ctypes
import os
import sys
import time

import numpy

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import blueberry_amd as bb  # noqa: E402
from blueberry_amd import _lib  # noqa: E402
from blueberry_amd.solver import HipEngine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=24926)
ap.add_argument("--dtype", default="float32")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--n-iter", type=int, default=100)
ap.add_argument("--rounds", type=int, default=8)
a = ap.parse_args()
HBM_BYTES_PER_MS = 8e12 / 1e3


def stats(t):
    t = numpy.asarray(t, dtype=numpy.float64)
    return "%9.4f ms (min %.4f max %.4f, %d calls)" % (numpy.median(t), t.min(), t.max(), t.size)


n = a.n
xs = numpy.cumsum(numpy.random.default_rng(0).standard_normal((n, 3)), axis=0)
x0 = xs + 0.5 * numpy.random.default_rng(1).standard_normal(xs.shape)
counts = numpy.empty((n, n))
for r0 in range(0, n, 2048):                              # row blocks: no (n, n, 3) temporary
    d = numpy.sqrt(((xs[r0:r0 + 2048, None, :] - xs[None, :, :]) ** 2).sum(axis=2))
    counts[r0:r0 + 2048] = numpy.where(d > 0, d, 1.0) ** -3.4
numpy.fill_diagonal(counts, 0.0)
cm = bb.ContactMap.from_matrix(counts, device=0)
cm._resident()
del counts

eng = HipEngine(n, a.dtype)
eng.set_wish_resident(cm, "counts", 3.0)
lay = eng.layout()
unit_bytes = (lay["u_end"] - lay["u_begin"]) * 8192      # the raw units: what both passes read
eng.set_coords(x0)
eng.set_timing(1)
times = {}
for name, call in (("score", lambda: eng.score(x0)), ("loglog", lambda: eng.loglog(x0))):
    call()
    t = []
    for _ in range(a.reps):
        out = call()
        t.append(eng.score_timing())
    times[name] = numpy.array(t)
pairs = int(out[:, 0].sum())
print("N=%d %s: %d pairs with a logarithm, %.1f MB of units" % (n, a.dtype, pairs, unit_bytes / 1e6), flush=True)
for name in ("score", "loglog"):
    t = times[name]
    print("  %-6s profile %s\n         fold    %s" % (name, stats(t[:, 0]), stats(t[:, 1])), flush=True)
    med = numpy.median(t[:, 0])
    print("         profile kernel: %.1f GB/s of units = %.3f of 8 TB/s; %.2f Gpairs/s"
          % (unit_bytes / med / 1e6, unit_bytes / med / HBM_BYTES_PER_MS, pairs / med / 1e6), flush=True)

t = []
for k in range(a.reps + 1):
    p = 0.9 if k % 2 == 0 else 1.0 / 0.9                  # back and forth: the values stay in range
    eng.sync()
    t0 = time.perf_counter()
    eng.repower(p)
    t.append((time.perf_counter() - t0) * 1e3)
print("  repower (call, %s path) %s" % (eng.iteration_path()[0], stats(t[1:])), flush=True)
eng.close()

# a read-write stream of as many bytes: a device-to-device copy by the HIP runtime the library has
# loaded (reads unit_bytes, writes unit_bytes), timed by HIP events
hip = ctypes.CDLL([q for q in _lib.hip_runtimes_loaded() if "libamdhip64" in q][0])


def hip_ok(rc):
    assert rc == 0, "HIP error %d" % rc


src, dst = ctypes.c_void_p(), ctypes.c_void_p()
hip_ok(hip.hipMalloc(ctypes.byref(src), ctypes.c_size_t(unit_bytes)))
hip_ok(hip.hipMalloc(ctypes.byref(dst), ctypes.c_size_t(unit_bytes)))
hip_ok(hip.hipMemset(src, 0, ctypes.c_size_t(unit_bytes)))
ev = [ctypes.c_void_p(), ctypes.c_void_p()]
for e in ev:
    hip_ok(hip.hipEventCreate(ctypes.byref(e)))
t = []
for k in range(a.reps + 1):
    hip_ok(hip.hipEventRecord(ev[0], None))
    hip_ok(hip.hipMemcpyAsync(dst, src, ctypes.c_size_t(unit_bytes), 3, None))   # device to device
    hip_ok(hip.hipEventRecord(ev[1], None))
    hip_ok(hip.hipEventSynchronize(ev[1]))
    ms = ctypes.c_float()
    hip_ok(hip.hipEventElapsedTime(ctypes.byref(ms), ev[0], ev[1]))
    t.append(ms.value)
for e in ev:
    hip_ok(hip.hipEventDestroy(e))
hip_ok(hip.hipFree(src))
hip_ok(hip.hipFree(dst))
med = float(numpy.median(t[1:]))
print("  read-write stream of %.1f MB (device-to-device copy) %s: %.1f GB/s read + written = %.3f of 8 TB/s"
      % (unit_bytes / 1e6, stats(t[1:]), 2 * unit_bytes / med / 1e6, 2 * unit_bytes / med / HBM_BYTES_PER_MS),
      flush=True)

for label, alpha in (("fixed alpha = 3", 3.0), ("alpha = ('auto', 3.0, %d)" % a.rounds, ("auto", 3.0, a.rounds))):
    t = []
    for k in range(3):
        s = bb.StructureSolver(n_iter=a.n_iter, dtype=a.dtype, alpha=alpha)
        t0 = time.perf_counter()
        s.fit(cm, init=x0)
        t.append((time.perf_counter() - t0) * 1e3)
    print("  fit, n_iter = %d, %s: %s; alpha_ = %.4f, %d rounds"
          % (a.n_iter, label, stats(t[1:]), s.alpha_, len(s.alpha_rounds_)), flush=True)
