"""Cost of `ContactMap.balance` / `ContactMap.expected` (docs/SPEC.md 2.5.2) on a
resident Hi-C-like map (tests/_balance_model.hic_like_raw), by default d = 24,927 (chr1 at 10 kb):

  * synchronised wall clock, warm, medians: the time per iteration of the balancing loop (the
    difference of a 30-update and a 10-update call over 20), one `bb_cm_symv` call, the diagonal
    pass with and without a bias vector, the whole `balance(tol=1e-5)`, and the numpy model's time
    for that same call on this host's threads;
  * with --kernels the tool runs itself once under `rocprofv3 --kernel-trace --stats` (a run of
    its own: no wall clock is taken there) and prints the average time of every kernel of the two
    calls next to symv's, with the bytes of the upper triangle over that time.

    python tools/balance_timing.py [--kernels] [--out FILE] [d]

The lines are printed and written to FILE (default profiles/balance_timing.txt; --kernels
appends)."""
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy

LINES = []


def say(line):
    print(line, flush=True)
    LINES.append(line)


def timed(fn):
    t0 = time.perf_counter()
    fn()                                                   # every call here ends synchronised
    return time.perf_counter() - t0


def median_of(fn, k):
    return statistics.median(timed(fn) for _ in range(k))


def symv(dev, x, y):
    from blueberry_amd import _lib
    _lib.check(dev._lib.bb_cm_symv(dev._h, _lib.as_f64_ptr(x), _lib.as_f64_ptr(y)), "bb_cm_symv")


def resident_map(d):
    import blueberry_amd as bb
    from tests import _balance_model as bm
    t0 = time.perf_counter()
    m = bm.hic_like_raw(d)
    cm = bb.ContactMap.from_matrix(m)
    cm._resident()
    say("d = %d (%d bins, %.2f GB matrix, %.2f GB upper triangle); map drawn and uploaded in %.1f s"
        % (d, d - 1, 8.0 * d * d / 1e9, 4.0 * (d - 1) * d / 1e9, time.perf_counter() - t0))
    return m, cm


def main(d):
    from tests import _balance_model as bm
    m, cm = resident_map(d)
    dev = cm._resident()
    pair_bytes = 4.0 * (d - 1) * d                         # 8 B per pair of the n x n upper triangle
    x, y = numpy.ones(d), numpy.empty(d)
    # warm: every kernel once, the scratch allocated
    cm.balance(tol=0.0, max_iter=2)
    cm.expected(bias=None)
    cm.expected()
    symv(dev, x, y)
    t10 = median_of(lambda: cm.balance(tol=0.0, max_iter=10), 5)
    t30 = median_of(lambda: cm.balance(tol=0.0, max_iter=30), 5)
    per_it = (t30 - t10) / 20.0
    say("balance, one iteration (product, reduce, step; (30 updates - 10 updates) / 20): %.1f us = "
        "%.2f TB/s of the upper triangle; the 10-update call %.2f ms, the 30-update call %.2f ms"
        % (per_it * 1e6, pair_bytes / per_it / 1e12, t10 * 1e3, t30 * 1e3))
    t_symv = median_of(lambda: symv(dev, x, y), 20)
    say("bb_cm_symv, one call (two vector copies and two allocations included): %.1f us" % (t_symv * 1e6))
    bias = cm.balance(ignore_diags=2, min_nnz=10)
    t_e1 = median_of(lambda: cm.expected(bias=bias), 10)
    t_e0 = median_of(lambda: cm.expected(bias=None), 10)
    say("expected, one call (diagonal pass, reduce, two vector copies): with a bias %.1f us = %.2f "
        "TB/s, without %.1f us = %.2f TB/s" % (t_e1 * 1e6, pair_bytes / t_e1 / 1e12, t_e0 * 1e6,
                                               pair_bytes / t_e0 / 1e12))
    t_bal = median_of(lambda: cm.balance(ignore_diags=2, min_nnz=10, tol=1e-5), 5)
    say("balance(ignore_diags=2, min_nnz=10, tol=1e-5): %.2f ms, %d updates, var %.3e, %d bins masked"
        % (t_bal * 1e3, cm.balance_iterations_, cm.balance_variance_, int(cm.balance_masked_.sum())))
    t0 = time.perf_counter()
    want = bm.balance(m, 2, 10, 1e-5, 200)
    t_model = time.perf_counter() - t0
    live = ~want["masked"]
    err = float(numpy.max(numpy.abs(bias[live] / want["bias"][live] - 1.0)))
    say("the numpy model of that call on this host (%s threads): %.2f s, %d updates; largest relative "
        "difference of b %.2e; device %.0fx faster"
        % (os.environ.get("OMP_NUM_THREADS", "all"), t_model, want["iterations"], err, t_model / t_bal))


def one(d):
    """What the --kernels child runs."""
    m, cm = resident_map(d)
    dev = cm._resident()
    x, y = numpy.ones(d), numpy.empty(d)
    for _ in range(2):
        bias = cm.balance(ignore_diags=2, tol=0.0, max_iter=20)
        cm.expected(bias=bias)
        cm.expected(bias=None)
        for _ in range(10):
            symv(dev, x, y)


def kernels(d):
    import csv
    import glob
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--",
               sys.executable, os.path.abspath(__file__), "--one", str(d)]
        run = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
        if run.returncode != 0:
            print(run.stdout.decode("utf-8", "replace")[-2000:])
            raise SystemExit("rocprofv3 run failed (status %d)" % run.returncode)
        files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        rows = [r for f in files for r in csv.DictReader(open(f))]
    pair_bytes = 4.0 * (d - 1) * d
    say("kernel times at d = %d under rocprofv3 --kernel-trace --stats (a run of its own):" % d)
    wanted = ("symv_upper_kernel", "band_symv_kernel", "symv_reduce_kernel", "balance_step_kernel",
              "balance_mask_kernel", "diag_sums_kernel", "diag_reduce_kernel")
    for r in sorted(rows, key=lambda r: r["Name"]):
        if not any(w in r["Name"] for w in wanted):
            continue
        avg = float(r["AverageNs"])
        sweep = any(w in r["Name"] for w in ("symv_upper", "band_symv", "diag_sums"))
        say("    %-70s calls %4s  avg %9.1f us%s"
            % (r["Name"][:70], r["Calls"], avg / 1e3,
               "  %.2f TB/s of the upper triangle" % (pair_bytes / (avg * 1e-9) / 1e12) if sweep else ""))


if __name__ == "__main__":
    args = sys.argv[1:]
    out = os.path.join(ROOT, "profiles", "balance_timing.txt")
    if "--out" in args:
        i = args.index("--out")
        out = args[i + 1]
        del args[i:i + 2]
    if args[:1] == ["--one"]:
        one(int(args[1]))
    else:
        want_kernels = args[:1] == ["--kernels"]
        size = int((args[1:] if want_kernels else args)[0]) if (args[1:] if want_kernels else args) else 24927
        (kernels if want_kernels else main)(size)
        with open(out, "a" if want_kernels else "w") as fh:
            fh.write("\n".join(LINES) + "\n")
