"""Cost of the landmark constraints inside the fit (docs/SPEC.md 2.5.5), warm,
fp32, L = 64 landmarks, on the two triple lists tools/landmark_timing.py uses:

  * the Hi-C-like map of tests/_balance_model.hic_like_raw at d = 24,927 (chr1 at 10 kb);
  * the synthetic whole-genome-sized list (tools/triples_balance_timing.synthetic): N bins
    (default 309,568: config 5) and PAIRS triples (default 2e8).  Its random far pairs name nearly
    every tile (190 GB of units), so the solver that carries ITS anchors holds BASELINE config 5's
    map instead -- the genome as blocks (tools/score_timing.py: 10.5 GB of units, wish distances
    generated on the device): the geodesics come from the list, the sweep beside them is the
    whole-genome sweep.

One solver per list holds the map and the anchors.  Reported, each the median (min..max) of
`--reps` blocks of `--steps` iterations timed by HIP events (bb_solver_set_timing), the data
resident and two blocks of warm-up first:
  anchored iteration     sweep | reduce + the three anchor launches + update, and the whole step
  unanchored iteration   the SAME solver with its anchors cleared, in the same run, after
                         the anchored blocks
  the anchor launches    alone, back to back (bb_solver_measure_anchors)
  their bytes            the rows are read twice (node side, landmark side): 2 L' n_pad 4 B, next
                         to the time the library's own read-only sweep (bb_solver_measure_stream_read)
                         would need for them at the rate it reaches on this solver's units

    python tools/anchor_timing.py [--out FILE] [--d D] [--bins N] [--pairs PAIRS] [--reps R] [--steps K]

--d 0 or --pairs 0 skips that input.  The lines are printed and written to FILE (default
profiles/anchor_timing.txt)."""
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
WEIGHT = 0.1


def say(line):
    print(line, flush=True)
    LINES.append(line)


def med(v):
    return "%.4f ms (min %.4f max %.4f)" % (statistics.median(v), min(v), max(v))


def blocks(eng, reps, steps, lr):
    """reps blocks of `steps` event-timed iterations: lists of sweep, rest and step times (ms)."""
    sweep, rest, step = [], [], []
    for _ in range(reps):
        eng.set_timing(1)
        eng.iterate(steps, lr)
        eng.sync()
        t = eng.timing()
        sweep.append(t["grad_ms"]), rest.append(t["reduce_ms"]), step.append(t["step_ms"])
    eng.set_timing(0)
    return sweep, rest, step


def time_anchors(t, n_nodes, reps, steps, genome=False):
    import blueberry_amd as bb
    from blueberry_amd.solver import HipEngine, landmark_choice, tiles_from_blocks, weighted_steps
    from blueberry_amd.utils import genome_boundaries
    dev = bb.DeviceTriples(t, RES, 0)
    graph = dict(kind="counts", alpha=3.0)
    live = numpy.flatnonzero(dev.edge_degrees(n_nodes, **graph) > 0)
    marks = landmark_choice(live, L)
    x0 = numpy.cumsum(numpy.random.default_rng(0).standard_normal((n_nodes, 3)), axis=0)
    if genome:
        tiles, _ = tiles_from_blocks(n_nodes, genome_boundaries(n_nodes), 1000, "float32")
        eng = HipEngine(n_nodes, "float32", tiles=tiles)
        eng.set_wish_from_coords(x0 + 0.5 * numpy.random.default_rng(1).standard_normal(x0.shape))
    else:
        eng = HipEngine(n_nodes, "float32", tiles=dev.tiles(n_nodes, "float32"))
        eng.set_wish_triples(dev, "counts", 3.0)
    rows = dev.shortest_paths(n_nodes, marks, **graph)
    t0 = time.perf_counter()
    eng.set_anchors(rows, None, WEIGHT)
    t_set = time.perf_counter() - t0
    rows.close()
    dev.close()
    kept, terms, nbytes = eng.anchor_info()
    n_pad = eng.layout()["n_pad"]
    sums = eng.degrees().astype(numpy.float64) + eng.anchor_sums()
    lr, scale = weighted_steps(sums, n_nodes, "float32", "auto", True)
    eng.set_bin_steps(scale)
    eng.set_coords(x0)
    unit_bytes = eng.traffic()["unit_bytes"]
    say("    %d nodes (n_pad %d), %d live, %.1f MB of units, path %s; %d kept rows, %d terms, %.1f MB "
        "resident; set_anchors (convert + copy, wall) %.2f ms"
        % (n_nodes, n_pad, live.size, unit_bytes / 1e6, eng.iteration_path()[0], kept, terms, nbytes / 1e6,
           t_set * 1e3))
    blocks(eng, 2, steps, lr)                               # warm-up
    a_sweep, a_rest, a_step = blocks(eng, reps, steps, lr)
    alone = [eng.anchor_ms(steps) for _ in range(reps)]
    read = [eng.stream_read_ms(10) for _ in range(max(3, reps // 2))]
    eng.set_anchors(None)
    blocks(eng, 2, steps, lr)
    p_sweep, p_rest, p_step = blocks(eng, reps, steps, lr)
    eng.close()
    say("    anchored iteration:   sweep %s; reduce + anchors + update %s; step %s"
        % (med(a_sweep), med(a_rest), med(a_step)))
    say("    unanchored iteration: sweep %s; reduce + update %s; step %s (the same solver, its anchors "
        "cleared)" % (med(p_sweep), med(p_rest), med(p_step)))
    anchor_bytes = 2.0 * kept * n_pad * 4
    rate = unit_bytes / (statistics.median(read) * 1e-3)
    say("    the three anchor launches alone: %s; the rows are read twice: %.1f MB = %.4f ms at the "
        "%.2f TB/s the read-only sweep reaches on this solver's units (%s)"
        % (med(alone), anchor_bytes / 1e6, anchor_bytes / rate * 1e3, rate / 1e12, med(read)))
    say("    anchored / unanchored step: %.3f" % (statistics.median(a_step) / statistics.median(p_step)))


def hic_input(d, reps, steps):
    from tests import _balance_model as bm
    from tests import _triples_model as tm
    t0 = time.perf_counter()
    t = tm.triples_of_matrix(bm.hic_like_raw(d), RES, border=False)
    say("Hi-C-like map, d = %d; drawn in %.1f s" % (d, time.perf_counter() - t0))
    time_anchors(t, d, reps, steps)


def synthetic_input(n, pairs, reps, steps):
    from tools.triples_balance_timing import synthetic
    t0 = time.perf_counter()
    t = synthetic(n, pairs)
    say("synthetic list, %d bins, %d triples; drawn in %.1f s" % (n, pairs, time.perf_counter() - t0))
    time_anchors(t, n + 1, reps, steps, genome=True)


if __name__ == "__main__":
    args = sys.argv[1:]
    opts = {"--out": os.path.join(ROOT, "profiles", "anchor_timing.txt"), "--d": "24927",
            "--bins": "309568", "--pairs": "200000000", "--reps": "9", "--steps": "20"}
    while args:
        if args[0] not in opts or len(args) < 2:
            raise SystemExit(__doc__)
        opts[args[0]] = args[1]
        del args[:2]
    reps, steps = int(opts["--reps"]), int(opts["--steps"])
    if int(opts["--d"]):
        hic_input(int(opts["--d"]), reps, steps)
    if int(float(opts["--pairs"])):
        synthetic_input(int(opts["--bins"]), int(float(opts["--pairs"])), reps, steps)
    os.makedirs(os.path.dirname(os.path.abspath(opts["--out"])), exist_ok=True)
    with open(opts["--out"], "w") as fh:
        fh.write("\n".join(LINES) + "\n")
