"""Cost of balancing straight from triples (`DeviceTriples.balance` / `.expected`, docs/SPEC.md
2.5.3), synchronised wall clock, warm, medians:

  * the Hi-C-like map of tests/_balance_model.hic_like_raw at d = 24,927 (chr1 at 10 kb) as
    triples, next to `ContactMap.balance` on the same map resident as a dense matrix: the index
    build (the first call on a fresh handle), the time per iteration of the loop (the difference
    of a 30-update and a 10-update call over 20) on both paths, the whole `balance(tol=1e-5)` on
    both, the expected;
  * a synthetic whole-genome-sized list: N bins (default 309,568: config 5), every pair within
    24 of the diagonal plus random far pairs up to PAIRS triples (default 2.54e9: config 5; a
    duplicate among the far pairs is legal -- the last wins -- and the stored pairs are
    reported): the same figures, triples alone;
  * the product's achieved bytes/s -- 12 B per directed entry over the time per iteration, which
    also holds the reduce and the step -- against the stream-read figure of
    `bb_solver_measure_stream_read` on the same device.

    python tools/triples_balance_timing.py [--kernels 1] [--out FILE] [--d D] [--bins N] [--pairs PAIRS]

--d 0 or --pairs 0 skips that input.  With --kernels 1 the tool runs itself under `rocprofv3
--kernel-trace --stats`, once per input (runs of their own: no wall clock is taken there), and
prints the average time of every kernel of the loop and of the expected, the product's with the
bytes of the index over that time.  The lines are printed and written to FILE (default
profiles/triples_balance_timing.txt; --kernels appends)."""
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
RES = 10000


def say(line):
    print(line, flush=True)
    LINES.append(line)


def timed(fn):
    t0 = time.perf_counter()
    fn()                                                   # every call here ends synchronised
    return time.perf_counter() - t0


def median_of(fn, k):
    return statistics.median(timed(fn) for _ in range(k))


def stream_read_rate():
    """bytes/s of the solver's read-only sweep over its resident units (fp32, 16,384 bins)."""
    from blueberry_amd.solver import HipEngine, layout_info
    n = 16384
    rng = numpy.random.default_rng(0)
    eng = HipEngine(n, "float32")
    eng.set_wish_from_coords(numpy.cumsum(rng.normal(size=(n, 3)), axis=0))
    eng.stream_read_ms(3)
    ms = eng.stream_read_ms(20)
    eng.close()
    return layout_info(n, "float32")["n_units"] * 8192.0 / (ms * 1e-3)


def time_triples(t, n, stream_rate, balance_kw):
    """The figures of one triple list; returns (time per iteration, time of the whole balance)."""
    import blueberry_amd as bb
    dev = bb.DeviceTriples(t, RES, 0)
    t_index = timed(lambda: dev.pairs(n))
    pairs = dev.pairs(n)
    say("    %d triples (%.2f GB), %d stored pairs; index build (first call on the handle): %.1f ms"
        % (t.shape[0], t.nbytes / 1e9, pairs, t_index * 1e3))
    dev.balance(n, tol=0.0, max_iter=2)                    # warm
    t10 = median_of(lambda: dev.balance(n, tol=0.0, max_iter=10), 5)
    t30 = median_of(lambda: dev.balance(n, tol=0.0, max_iter=30), 5)
    per_it = (t30 - t10) / 20.0
    # directed entries: two per pair off the diagonal, one on it; the diagonal's share is below
    # n / pairs, so 2 pairs - (stored diagonal cells <= n) is bracketed, and reported as such
    lo, hi = 12.0 * (2 * pairs - n), 12.0 * 2 * pairs
    say("    triples, one iteration (product, reduce, step; (30 updates - 10 updates) / 20): %.1f us "
        "= %.3f to %.3f TB/s of the index (12 B per directed entry), %.0f %% of the stream-read "
        "figure %.2f TB/s" % (per_it * 1e6, lo / per_it / 1e12, hi / per_it / 1e12,
                              100.0 * hi / per_it / stream_rate, stream_rate / 1e12))
    t_bal = median_of(lambda: dev.balance(n, **balance_kw), 5)
    bias = dev.balance(n, **balance_kw)
    say("    triples, balance(%s): %.2f ms, %d updates, var %.3e, %d bins masked"
        % (", ".join("%s=%r" % kv for kv in sorted(balance_kw.items())), t_bal * 1e3,
           dev.balance_iterations_, dev.balance_variance_, int(dev.balance_masked_.sum())))
    t_first = timed(lambda: dev.expected(n, bias))
    t_e = median_of(lambda: dev.expected(n, bias), 5)
    say("    triples, expected: first call (builds the diagonal ordering) %.1f ms, then %.1f us"
        % (t_first * 1e3, t_e * 1e6))
    dev.close()
    return per_it, t_bal, bias


def hic_input(d, stream_rate):
    import blueberry_amd as bb
    from tests import _balance_model as bm
    from tests import _triples_model as tm
    t0 = time.perf_counter()
    m = bm.hic_like_raw(d)
    t = tm.triples_of_matrix(m, RES, border=False)
    say("Hi-C-like map, d = %d (%d bins; dense %.2f GB, upper triangle %.2f GB); drawn in %.1f s"
        % (d, d - 1, 8.0 * d * d / 1e9, 4.0 * (d - 1) * d / 1e9, time.perf_counter() - t0))
    kw = dict(ignore_diags=2, min_nnz=10, tol=1e-5)
    per_it, t_bal, bias = time_triples(t, d - 1, stream_rate, kw)
    cm = bb.ContactMap.from_matrix(m)
    cm.balance(tol=0.0, max_iter=2)
    d10 = median_of(lambda: cm.balance(tol=0.0, max_iter=10), 5)
    d30 = median_of(lambda: cm.balance(tol=0.0, max_iter=30), 5)
    dense_it = (d30 - d10) / 20.0
    d_bal = median_of(lambda: cm.balance(**kw), 5)
    dense = cm.balance(**kw)
    live = ~numpy.isnan(dense)
    say("    dense, one iteration: %.1f us (%.2f TB/s of the upper triangle); balance: %.2f ms, %d "
        "updates; triples / dense per iteration %.2f, whole call %.2f; largest relative "
        "difference of b %.2e"
        % (dense_it * 1e6, 4.0 * (d - 1) * d / dense_it / 1e12, d_bal * 1e3, cm.balance_iterations_,
           per_it / dense_it, t_bal / d_bal, float(numpy.max(numpy.abs(bias[live] / dense[live] - 1.0)))))


def synthetic(n, pairs, seed=5):
    """Every pair within 24 of the diagonal, then random far pairs, `pairs` rows in all."""
    rng = numpy.random.default_rng(seed)
    band = min(pairs, 25 * n)
    t = numpy.empty((pairs, 3))
    k = numpy.arange(band)
    i, off = k // 25, k % 25
    j = numpy.minimum(i + off, n - 1)
    t[:band, 0], t[:band, 1] = i * float(RES), j * float(RES)
    step = 1 << 26
    for a in range(band, pairs, step):                     # (in pieces: no second copy)
        b = min(pairs, a + step)
        t[a:b, 0] = rng.integers(0, n, size=b - a) * float(RES)
        t[a:b, 1] = rng.integers(0, n, size=b - a) * float(RES)
        t[a:b, 2] = rng.integers(1, 8, size=b - a)
    t[:band, 2] = rng.integers(1, 200, size=band)
    return t


def synthetic_input(n, pairs, stream_rate):
    t0 = time.perf_counter()
    t = synthetic(n, pairs)
    say("synthetic list, %d bins, %d triples; drawn in %.1f s" % (n, pairs, time.perf_counter() - t0))
    time_triples(t, n, stream_rate, dict(tol=1e-5))


def one(which, d, n, pairs):
    """What a --kernels child runs: 2 x (20 updates, the expected with and without a bias)."""
    import blueberry_amd as bb
    if which == "hic":
        from tests import _balance_model as bm
        from tests import _triples_model as tm
        t, n = tm.triples_of_matrix(bm.hic_like_raw(d), RES, border=False), d - 1
    else:
        t = synthetic(n, pairs)
    dev = bb.DeviceTriples(t, RES, 0)
    for _ in range(2):
        bias = dev.balance(n, tol=0.0, max_iter=20)
        dev.expected(n, bias)
        dev.expected(n)
    print("PAIRS %d" % dev.pairs(n))
    dev.close()


def kernels(which, d, n, pairs, stream_rate):
    import csv
    import glob
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--",
               sys.executable, os.path.abspath(__file__), "--one", which, "--d", str(d), "--bins", str(n),
               "--pairs", str(pairs)]
        run = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
        text = run.stdout.decode("utf-8", "replace")
        if run.returncode != 0:
            print(text[-2000:])
            raise SystemExit("rocprofv3 run failed (status %d)" % run.returncode)
        files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        rows = [r for f in files for r in csv.DictReader(open(f))]
    stored = int(text.split("PAIRS ")[1].split()[0])
    index_bytes = 24.0 * stored                           # (12 B per directed entry, diagonal cells once: an upper bound)
    say("kernel times, %s input (%d stored pairs), under rocprofv3 --kernel-trace --stats (a run of "
        "its own):" % (which, stored))
    wanted = ("seg_sum_kernel", "seg_reduce_kernel", "balance_step_kernel", "balance_mask_kernel",
              "pair_counts_kernel", "pack_live_kernel")
    for r in sorted(rows, key=lambda r: r["Name"]):
        if not any(w in r["Name"] for w in wanted):
            continue
        avg = float(r["AverageNs"])
        rate = ""
        if "seg_sum_kernel<0>" in r["Name"] or "seg_sum_kernel<(int)0>" in r["Name"]:
            rate = "  %.2f TB/s of the index, %.0f %% of the stream-read figure" % (
                index_bytes / (avg * 1e-9) / 1e12, 100.0 * index_bytes / (avg * 1e-9) / stream_rate)
        say("    %-60s calls %4s  avg %9.1f us%s" % (r["Name"][:60], r["Calls"], avg / 1e3, rate))


if __name__ == "__main__":
    args = sys.argv[1:]
    opts = {"--out": os.path.join(ROOT, "profiles", "triples_balance_timing.txt"), "--d": "24927",
            "--bins": "309568", "--pairs": "2540000000", "--kernels": "0", "--one": ""}
    while args:
        if args[0] not in opts or len(args) < 2:
            raise SystemExit(__doc__)
        opts[args[0]] = args[1]
        del args[:2]
    if opts["--one"]:
        one(opts["--one"], int(opts["--d"]), int(opts["--bins"]), int(float(opts["--pairs"])))
        raise SystemExit(0)
    rate = stream_read_rate()
    say("stream read of the solver's resident units (bb_solver_measure_stream_read): %.2f TB/s" % (rate / 1e12))
    want_kernels = int(opts["--kernels"]) != 0
    if int(opts["--d"]):
        if want_kernels:
            kernels("hic", int(opts["--d"]), 0, 0, rate)
        else:
            hic_input(int(opts["--d"]), rate)
    if int(float(opts["--pairs"])):
        if want_kernels:
            kernels("synthetic", 0, int(opts["--bins"]), int(float(opts["--pairs"])), rate)
        else:
            synthetic_input(int(opts["--bins"]), int(float(opts["--pairs"])), rate)
    with open(opts["--out"], "a" if want_kernels else "w") as fh:
        fh.write("\n".join(LINES) + "\n")
