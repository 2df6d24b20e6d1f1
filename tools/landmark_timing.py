"""Cost of the landmark start's shortest paths (`DeviceTriples.shortest_paths`, `landmark_start`;
docs/SPEC.md 2.1.2 and 2.5.4), warm:

  * the Hi-C-like map of tests/_balance_model.hic_like_raw at d = 24,927 (chr1 at 10 kb) as
    triples, L = 64 landmarks: the index build, the weights pass and the sweeps by the HIP events
    of `bb_paths_timing`, the number of sweeps, the time per sweep with the bytes DESIGN 4.19
    counts for it (20 B per directed entry and 64-source chunk, 512 B of D per entry and wave),
    the placement and the whole `landmark_start` by synchronised wall clock -- next to
    `scipy.sparse.csgraph.dijkstra` from the same sources on this host (and the largest
    relative difference of the two results), and to `ContactMap.shortest_paths`, the dense
    completion, on the same map;
  * a synthetic whole-genome-sized list (tools/triples_balance_timing.synthetic): N bins (default
    309,568: config 5) and PAIRS triples (default 2e8), the device figures alone.

    python tools/landmark_timing.py [--out FILE] [--d D] [--bins N] [--pairs PAIRS] [--scipy 1] [--dense 1]

--d 0 or --pairs 0 skips that input; --scipy 0 / --dense 0 skip the two comparisons.  The lines
are printed and written to FILE (default profiles/landmark_timing.txt)."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy

LINES = []
RES = 10000
L = 64


def say(line):
    print(line, flush=True)
    LINES.append(line)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()                                             # every call here ends synchronised
    return time.perf_counter() - t0, out


def time_paths(t, n_nodes, kind):
    """The device figures of one triple list; returns (landmarks, their rows on the host)."""
    import blueberry_amd as bb
    from blueberry_amd.solver import landmark_choice
    dev = bb.DeviceTriples(t, RES, 0)
    graph = dict(kind=kind, alpha=3.0)
    t_index, deg = timed(lambda: dev.edge_degrees(n_nodes, **graph))
    t_deg, deg = timed(lambda: dev.edge_degrees(n_nodes, **graph))
    entries = int(deg.sum())
    live = numpy.flatnonzero(deg > 0)
    marks = landmark_choice(live, L)
    say("    %d triples (%.2f GB), %d nodes, %d live, %d directed edges; index build + degrees (first "
        "call on the handle): %.1f ms, degrees again: %.2f ms"
        % (t.shape[0], t.nbytes / 1e9, n_nodes, live.size, entries, t_index * 1e3, t_deg * 1e3))
    dev.shortest_paths(n_nodes, marks, **graph).close()    # warm
    runs = []
    for _ in range(3):
        wall, rows = timed(lambda: dev.shortest_paths(n_nodes, marks, **graph))
        runs.append((wall,) + rows.timing() + (rows.sweeps_,))
        rows.close()
    rows = dev.shortest_paths(n_nodes, marks, **graph)
    wall = statistics.median(r[0] for r in runs)
    w_ms = statistics.median(r[1] for r in runs)
    per = statistics.median(r[2] / max(r[3], 1) for r in runs)
    chunks = (len(marks) + 63) // 64
    sweep_bytes = entries * chunks * (20.0 + 512.0)
    say("    shortest paths from %d landmarks: %.2f ms the call; weights %.3f ms; sweeps %s (not "
        "reproducible), %.3f ms per sweep = %.2f TB/s of DESIGN 4.19's bytes (%.2f GB per sweep, of "
        "which D rows %.2f GB); %d unreachable"
        % (len(marks), wall * 1e3, w_ms, "/".join(str(r[3]) for r in runs), per,
           sweep_bytes / (per * 1e-3) / 1e12, sweep_bytes / 1e9, entries * chunks * 512.0 / 1e9,
           rows.unreachable_))
    G = rows.columns(marks)
    coef, mu = bb.landmark_coefficients(G)
    rows.place(coef, mu)
    t_place = statistics.median(timed(lambda: rows.place(coef, mu))[0] for _ in range(3))
    say("    placement of %d nodes (upload, kernel, download, wall): %.2f ms" % (n_nodes, t_place * 1e3))
    host = rows.to_host() if n_nodes <= 50000 else None
    rows.close()
    t_all = statistics.median(timed(lambda: bb.landmark_start(dev, RES, n_nodes - 1, n_landmarks=L, **graph))[0]
                              for _ in range(3))
    say("    landmark_start on the open handle (degrees, paths, eigh of %d x %d, placement): %.2f ms"
        % (len(marks), len(marks), t_all * 1e3))
    dev.close()
    return marks, host


def hic_input(d, want_scipy, want_dense):
    import blueberry_amd as bb
    from tests import _balance_model as bm
    from tests import _triples_model as tm
    t0 = time.perf_counter()
    m = bm.hic_like_raw(d)
    t = tm.triples_of_matrix(m, RES, border=False)
    say("Hi-C-like map, d = %d (dense %.2f GB); drawn in %.1f s" % (d, 8.0 * d * d / 1e9, time.perf_counter() - t0))
    marks, host = time_paths(t, d, "counts")
    if want_scipy:
        import scipy.sparse
        import scipy.sparse.csgraph
        i, j = (t[:, 0] / RES).astype(numpy.int64), (t[:, 1] / RES).astype(numpy.int64)
        ok = (i != j) & (t[:, 2] > 0)
        w = scipy.sparse.csr_matrix((t[ok, 2] ** (-1.0 / 3.0), (i[ok], j[ok])), shape=(d, d))
        t_sp, ref = timed(lambda: scipy.sparse.csgraph.dijkstra(w, directed=False, indices=marks))
        ref = numpy.where(numpy.isinf(ref), 0.0, ref)
        rel = numpy.abs(host - ref) / numpy.maximum(ref, 1e-300)
        say("    scipy.sparse.csgraph.dijkstra from the same %d sources on this host: %.2f s; largest "
            "relative difference of the device's rows %.2e (pow() on the device, numpy's here)"
            % (len(marks), t_sp, float(rel.max())))
    if want_dense:
        cm = bb.ContactMap.from_matrix(m)
        first, out = timed(lambda: cm.shortest_paths(alpha=3.0, kind="counts"))
        del out
        again, out = timed(lambda: cm.shortest_paths(alpha=3.0, kind="counts"))
        say("    ContactMap.shortest_paths (dense completion, all %d x %d pairs): %.2f s the first "
            "call, %.2f s the second" % (d, d, first, again))


def synthetic_input(n, pairs):
    from tools.triples_balance_timing import synthetic
    t0 = time.perf_counter()
    t = synthetic(n, pairs)
    say("synthetic list, %d bins, %d triples; drawn in %.1f s" % (n, pairs, time.perf_counter() - t0))
    time_paths(t, n + 1, "counts")


if __name__ == "__main__":
    args = sys.argv[1:]
    opts = {"--out": os.path.join(ROOT, "profiles", "landmark_timing.txt"), "--d": "24927",
            "--bins": "309568", "--pairs": "200000000", "--scipy": "1", "--dense": "1"}
    while args:
        if args[0] not in opts or len(args) < 2:
            raise SystemExit(__doc__)
        opts[args[0]] = args[1]
        del args[:2]
    if int(opts["--d"]):
        hic_input(int(opts["--d"]), int(opts["--scipy"]) != 0, int(opts["--dense"]) != 0)
    if int(float(opts["--pairs"])):
        synthetic_input(int(opts["--bins"]), int(float(opts["--pairs"])))
    os.makedirs(os.path.dirname(os.path.abspath(opts["--out"])), exist_ok=True)
    with open(opts["--out"], "w") as fh:
        fh.write("\n".join(LINES) + "\n")
