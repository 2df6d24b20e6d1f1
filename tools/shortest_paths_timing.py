"""Cost of the shortest-path completion (bb_cm_shortest_paths, docs/SPEC.md 2.1.1) on a map
that is already resident: per size the synchronised wall clock of the call (1 warm-up, median
of 5), N^3 min-plus relaxations per second, and the bytes the third phase moves per round,
so that a reader can see which side of the roofline it sits on.  Then
  * N = 2,000: the whole host-to-host call (upload and download included) against
    scipy.sparse.csgraph.shortest_path(method='FW') on the same matrix on this host;
  * the largest size: the 100 fp32 iterations the completion precedes, from the completed map.
With --phases the tool runs itself once per size under `rocprofv3 --kernel-trace --stats` (a run
of its own: no timing is taken there) and prints the share of each kernel.
    python tools/shortest_paths_timing.py [--phases] [n_bins ...]"""
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy

TILE = 64      # kFT of bb_shortest.hip: tile edge = k-depth of a round


def banded_map(n, device=0):
    """A resident map with a count for every pair at most 8 bins apart (the run time of a
    Floyd-Warshall pass does not depend on the values)."""
    import blueberry_amd as bb
    r = numpy.random.default_rng(n)
    rows = []
    for k in range(1, 9):
        i = numpy.arange(n - k, dtype=numpy.float64)
        rows.append(numpy.stack([i, i + k, r.integers(1, 200, size=n - k).astype(numpy.float64)], axis=1))
    return bb.ContactMap.from_triples(numpy.concatenate(rows), 1, n - 1, device=device)


def complete_once(src, dst):
    from blueberry_amd import _lib
    from blueberry_amd.datatypes import _shortest_paths_device
    t0 = time.perf_counter()
    _shortest_paths_device(src, dst, _lib.BB_KIND_COUNTS, 3.0)      # synchronous
    return time.perf_counter() - t0


def time_size(n):
    from blueberry_amd.datatypes import _DeviceMatrix
    cm = banded_map(n)
    src = cm._resident()
    dst = _DeviceMatrix(n, src.device)
    complete_once(src, dst)
    t = statistics.median(complete_once(src, dst) for _ in range(5))
    p = -(-n // TILE) * TILE
    rounds = p // TILE
    per_round = 8 * p * p                      # the third phase reads and writes every UPPER tile once
    print("N=%6d  completion %10.2f ms  %.3e relaxations/s (N^3 / time)  rounds %d  third phase "
          "%.3f GB per round, %.3f TB in all = %.2f TB/s if that alone set the time"
          % (n, t * 1e3, float(n) ** 3 / t, rounds, per_round / 1e9, rounds * per_round / 1e12,
             rounds * per_round / 1e12 / t))
    return cm, dst, t


def main(sizes):
    import blueberry_amd as bb
    from blueberry_amd.solver import HipEngine
    last = None
    for n in sizes:
        last = (n,) + time_size(n)
    # host to host against scipy's Floyd-Warshall
    import scipy.sparse.csgraph
    n = 2000
    with numpy.errstate(divide="ignore"):
        m = banded_map(n).to_host() ** (-1.0 / 3.0)
    m[~numpy.isfinite(m)] = 0.0
    bb.shortest_paths(m, kind="wish")
    t_dev = statistics.median(_timed(lambda: bb.shortest_paths(m, kind="wish")) for _ in range(5))
    t0 = time.perf_counter()
    ref = scipy.sparse.csgraph.shortest_path(m, method="FW", directed=False)
    t_ref = time.perf_counter() - t0
    g = bb.shortest_paths(m, kind="wish")
    err = float(numpy.abs(g - ref).max() / ref.max())
    print("N=%6d  host to host (upload, completion, download) %.2f ms; scipy shortest_path("
          "method='FW') on this host %.2f ms: %.0fx; largest difference %.1e of the longest path"
          % (n, t_dev * 1e3, t_ref * 1e3, t_ref / t_dev, err))
    # the iterations the completion precedes
    n, _, completed, t = last
    eng = HipEngine(n, "float32")
    eng.set_wish_from_cm(completed, "wish", 3.0)
    x0 = numpy.random.default_rng(0).standard_normal((n, 3))
    best = 1e9
    for _ in range(3):
        eng.set_coords(x0)
        eng.sync()
        t0 = time.perf_counter()
        eng.iterate(100, 1.0 / (2 * n))
        eng.sync()
        best = min(best, time.perf_counter() - t0)
    eng.close()
    print("N=%6d  completion %.1f ms; the 100 fp32 iterations it precedes %.1f ms" % (n, t * 1e3, best * 1e3))


def _timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def phases(sizes):
    """One completion per size under rocprofv3 --kernel-trace --stats, each a child process."""
    import csv
    import glob
    for n in sizes:
        with tempfile.TemporaryDirectory() as d:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
                   sys.executable, os.path.abspath(__file__), "--one", str(n)]
            run = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
            if run.returncode != 0:
                print(run.stdout.decode("utf-8", "replace")[-2000:])
                raise SystemExit("rocprofv3 run failed for N=%d (status %d)" % (n, run.returncode))
            files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
            rows = [r for f in files for r in csv.DictReader(open(f))]
        fw = [r for r in rows if "fw_" in r["Name"]]
        total = sum(float(r["TotalDurationNs"]) for r in fw)
        print("N=%6d  kernel time of one completion %.2f ms" % (n, total / 1e6))
        for r in sorted(fw, key=lambda r: -float(r["TotalDurationNs"])):
            name = r["Name"]
            phase = {"fw_diag_kernel": "phase 1, diagonal tile", "fw_panel_kernel": "phase 2, row panel",
                     "fw_tiles_kernel": "phase 3, all other tiles", "fw_load_kernel": "matrix -> work matrix",
                     "fw_store_kernel": "work matrix -> matrix"}
            label = next((v for k, v in phase.items() if k in name), name)
            print("    %-26s calls %5s  avg %10.2f us  total %10.2f ms  %5.1f %%"
                  % (label, r["Calls"], float(r["AverageNs"]) / 1e3, float(r["TotalDurationNs"]) / 1e6,
                     100.0 * float(r["TotalDurationNs"]) / total))


if __name__ == "__main__":
    args = sys.argv[1:]
    if args[:1] == ["--one"]:
        cm = banded_map(int(args[1]))
        out = cm.shortest_paths()
        print("N=%d unreachable pairs %d" % (int(args[1]), out.unreachable_pairs_))
    elif args[:1] == ["--phases"]:
        phases([int(v) for v in args[1:]] or [2000, 8192, 24926])
    else:
        main([int(v) for v in args] or [2000, 8192, 24926])
