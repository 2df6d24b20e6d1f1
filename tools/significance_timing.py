"""Cost of the Fit-Hi-C significance call (docs/SPEC.md 2.9) on a resident
Hi-C-like map (tests/_balance_model.hic_like_raw), by default d = 24,927 (chr1 at 10 kb) with the
default range (0, 10 Mb], dense and as triples.  Synchronised wall clock, warm, medians of 5; the
two device passes by the HIP events of the call itself (`bb_sig_timing`):

  * the tally (`bb_cm_expected` / `bb_triples_expected` with all weights 1);
  * the list (count, scan, write) and the p-value pass: cells per second, mean terms per cell;
  * the host's stable argsort of the p-values and the Benjamini-Hochberg scan: the q stage as it
    was before the device sort, timed here in the same process;
  * the device q stage (`bb_sig_q_values`): its two HIP-event times, the call and the read-back of
    q by wall clock, and host against device with their ranges over 5;
  * the whole `fit_transform`, without and with `q_max = 0.01`;
  * lane utilisation of the p-value pass, from the model's term counts of every 50th wave of the
    list (64 consecutive cells): sum of terms over 64 x sum of the waves' longest.

    python tools/significance_timing.py [--out FILE] [d [max_dist]]

The lines are printed and written to FILE (default profiles/significance_timing.txt)."""
import os
import statistics
import sys
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


def median_of(fn, k=5):
    return statistics.median(timed(fn) for _ in range(k))


def route(name, X, n, bias, max_dist, f_args):
    import blueberry_amd as bb
    from blueberry_amd import fithic as fh
    f = bb.FitHiC(resolution=RES, max_dist=max_dist)
    out = f.fit_transform(X, biases=bias, **f_args)                     # warm
    k_lo, k_hi = fh.in_range_diagonals(n, RES, f.min_dist, f.max_dist)
    t_tally = median_of(lambda: fh.diagonal_sums(X, n))
    say("%s: tally (diagonal sums, all weights 1): %.2f ms" % (name, t_tally * 1e3))
    lists, ps = [], []

    def device_pass():
        res = fh.significance_list(X, n, k_lo, k_hi, bias, f.bias_range, f.prior_by_distance_, f.n_reads_)
        a, b = res.timing()
        lists.append(a)
        ps.append(b)
        res.close()

    t_dev = median_of(device_pass)
    list_ms, p_ms = statistics.median(lists), statistics.median(ps)
    say("%s: device call %.2f ms: list (count, scan, write) %.3f ms; p-value pass %.3f ms (%.3f to %.3f "
        "over 5) = %.3g cells/s, %.1f terms per cell (%d listed of %d tests, %d reads)"
        % (name, t_dev * 1e3, list_ms, p_ms, min(ps), max(ps), f.n_listed_ / (p_ms * 1e-3),
           f.terms_ / max(f.n_listed_, 1), f.n_listed_, f.n_tests_, f.n_reads_))
    p = out.map[:, 3].copy()
    t_sort = median_of(lambda: numpy.argsort(p, kind="stable"))
    order = numpy.argsort(p, kind="stable")
    ps_sorted = p[order]
    t_bh = median_of(lambda: bb.benjamini_hochberg(ps_sorted, f.n_tests_))
    say("%s: host stable argsort of p %.1f ms; BH scan (upload, scan, download) %.1f ms"
        % (name, t_sort * 1e3, t_bh * 1e3))

    # the q stage both ways in this one process: the host route as fit_transform had it (argsort,
    # gather, bb.benjamini_hochberg, scatter; p already on the host) against the device route
    # (bb_sig_q_values on the resident list, and the read-back of q)
    def host_q():
        o = numpy.argsort(p, kind="stable")
        q = numpy.empty_like(p)
        q[o] = bb.benjamini_hochberg(p[o], f.n_tests_)
        return q

    host = [timed(host_q) for _ in range(5)]
    res = fh.significance_list(X, n, k_lo, k_hi, bias, f.bias_range, f.prior_by_distance_, f.n_reads_)
    res.q_values(f.n_tests_)                                            # warm
    same = numpy.array_equal(res.read_q().view(numpy.uint64), host_q().view(numpy.uint64))
    sorts, scans, calls, reads = [], [], [], []
    for _ in range(5):
        t0 = time.perf_counter()
        a, b = res.q_values(f.n_tests_)
        t1 = time.perf_counter()
        res.read_q()
        t2 = time.perf_counter()
        sorts.append(a), scans.append(b), calls.append(t1 - t0), reads.append(t2 - t1)
    res.close()
    dev = [c + r for c, r in zip(calls, reads)]
    med = statistics.median
    say("%s: device q stage: keys + sort %.3f ms, gather + scan + scatter %.3f ms (HIP events); the call "
        "%.2f ms, the read-back of q %.2f ms (wall clock, medians of 5); same bits as the host route: %s"
        % (name, med(sorts), med(scans), med(calls) * 1e3, med(reads) * 1e3, same))
    say("%s: q stage, host (argsort, gather, BH round trip, scatter) %.1f ms (%.1f to %.1f over 5); device "
        "(call + read-back) %.2f ms (%.2f to %.2f over 5): %.1f x, ranges %s"
        % (name, med(host) * 1e3, min(host) * 1e3, max(host) * 1e3, med(dev) * 1e3, min(dev) * 1e3,
           max(dev) * 1e3, med(host) / med(dev), "apart" if max(dev) < min(host) else "OVERLAP"))
    t_all = median_of(lambda: f.fit_transform(X, biases=bias, **f_args))
    t_sel = median_of(lambda: f.fit_transform(X, biases=bias, q_max=0.01, **f_args))
    say("%s: fit_transform %.1f ms (q stage on the device: sort %.3f + scan %.3f ms by its events); with "
        "q_max = 0.01 %.1f ms (%d selected of %d listed)"
        % (name, t_all * 1e3, f.sort_ms_, f.bh_ms_, t_sel * 1e3, f.n_selected_, f.n_listed_))
    return f, out


def utilisation(f, out, bias):
    from tests import _fithic_model as fm
    m = out.map
    row = ((m[:, 0] - RES // 2) / RES).astype(numpy.int64)
    col = ((m[:, 1] - RES // 2) / RES).astype(numpy.int64)
    waves = numpy.arange(0, m.shape[0] // 64, 50)
    pick = (waves[:, None] * 64 + numpy.arange(64)[None, :]).reshape(-1)
    pi = f.prior_by_distance_[col[pick] - row[pick]] * bias[row[pick]] * bias[col[pick]]
    _, terms = fm.binomial_sf(m[pick, 2].astype(numpy.int64), f.n_reads_, pi, return_terms=True)
    terms = numpy.maximum(terms, 1).reshape(-1, 64)
    say("p-value pass, lane utilisation over %d sampled waves: %.2f (terms: mean %.1f, mean of a wave's "
        "longest %.1f, longest %d)" % (terms.shape[0], terms.sum() / (64.0 * terms.max(axis=1).sum()),
                                       terms.mean(), terms.max(axis=1).mean(), terms.max()))


def main(d, max_dist):
    import blueberry_amd as bb
    from tests import _balance_model as bm
    from tests import _triples_model as tm
    n = d - 1
    t0 = time.perf_counter()
    m = bm.hic_like_raw(d)
    cm = bb.ContactMap.from_matrix(m, resolution=RES)
    cm._resident()
    say("d = %d (%d bins at %d bp, %.2f GB matrix), range (0, %d]; map drawn and uploaded in %.1f s"
        % (d, n, RES, 8.0 * d * d / 1e9, max_dist, time.perf_counter() - t0))
    bias = cm.balance(ignore_diags=2, min_nnz=10)
    f, out = route("dense", cm, n, bias, max_dist, {})
    utilisation(f, out, bias)
    t0 = time.perf_counter()
    t = tm.triples_of_matrix(m, RES, border=False)
    dev = bb.DeviceTriples(t, RES, 0)
    dev.pairs(n)
    say("triples: %d triples; list made, uploaded and indexed in %.1f s" % (t.shape[0], time.perf_counter() - t0))
    f2, out2 = route("triples", dev, n, bias, max_dist, {"map_bins": n})
    same = out.map.shape == out2.map.shape and numpy.array_equal(out.map.view(numpy.uint64),
                                                                   out2.map.view(numpy.uint64))
    say("the two routes' results are bit-identical: %s" % same)


if __name__ == "__main__":
    args = sys.argv[1:]
    out_file = os.path.join(ROOT, "profiles", "significance_timing.txt")
    if "--out" in args:
        i = args.index("--out")
        out_file = args[i + 1]
        del args[i:i + 2]
    main(int(args[0]) if args else 24927, int(args[1]) if len(args) > 1 else 10000000)
    with open(out_file, "w") as fh_:
        fh_.write("\n".join(LINES) + "\n")
