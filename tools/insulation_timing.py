"""Cost of the insulation sums of a map (docs/SPEC.md 2.13) on the Hi-C-like map
of tests/_balance_model.hic_like_raw, by default d = 24,927 (chr1 at 10 kb), for windows of 10, 25,
50 and 100 bins, ignore_diags = 2, no bias:

  * dense (`bb_cm_insulation`): the kernel by the handle's clock (`bb_cm_insulation_timing`), one
    warm call and the median (min..max) of `reps` calls; beside it the algorithmic bytes -- the
    band, about 16 n w: 8 bytes for each of the 2 n w cells within 2 w of the diagonal -- and
    what that is of the stream-read figure of `HipEngine.stream_read_ms` measured in the same
    process (a workgroup of 64 bins reads (63 + w)^2 cells, more than its share of the band);
  * pixel list (`bb_triples_insulation`): the map's non-zero cells as triples; the kernel by the
    handle's clock with the index already on the handle (`bb_triples_insulation_timing`), and
    the wall clock of the first call on a fresh handle, which builds the index, host to host --
    the host tail (`InsulationTrack`) included, and timed again on its own beside it.

    python tools/insulation_timing.py [d] [reps]

Not a test; bench.py does not call it."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy  # noqa: E402

import blueberry_amd as bb  # noqa: E402
from tests import _balance_model as bm  # noqa: E402
from tests import _triples_model as tm  # noqa: E402
from tools.coarsen_timing import say, spread, stream_read_rate, timed  # noqa: E402

RES = 10000
WINDOWS = (10, 25, 50, 100)
IGNORE = 2


def main(d, reps):
    n = d - 1
    rate = stream_read_rate()
    say("stream read (HipEngine.stream_read_ms, fp32 units of 16,384 bins): %.3f TB/s" % (rate / 1e12))
    m = bm.hic_like_raw(d)
    t = tm.triples_of_matrix(m, RES, border=False)
    cmap = bb.ContactMap.from_matrix(m, resolution=RES)
    cmap._resident()
    del m
    say("dense, d = %d (%.2f GB resident), ignore_diags = %d:" % (d, d * d * 8 / 1e9, IGNORE))
    dense = {}
    for w in WINDOWS:
        ms = [cmap.insulation(w, IGNORE, None).kernel_ms for _ in range(reps + 1)][1:]
        dense[w] = cmap.insulation(w, IGNORE, None)
        band = 16.0 * n * w
        got = band / (statistics.median(ms) * 1e-3)
        say("    window %-4d %s: band %.1f MB = %.3f TB/s = %.3f of the stream read; %d boundaries"
            % (w, spread(ms), band / 1e6, got / 1e12, got / rate, dense[w].boundaries()[0].shape[0]))
    cmap._dev.close()                                      # (the dense matrix leaves the device)
    del cmap
    say("pixel list, %d triples (%.2f GB):" % (t.shape[0], t.nbytes / 1e9))
    for w in WINDOWS:
        dev = bb.DeviceTriples(t, RES, 0)
        first, track = timed(lambda: dev.insulation(n, w, IGNORE))
        same = (numpy.array_equal(track.sums.view(numpy.uint64), dense[w].sums.view(numpy.uint64))
                and numpy.array_equal(track.counts, dense[w].counts))
        ms = [dev.insulation(n, w, IGNORE).kernel_ms for _ in range(reps + 1)][1:]
        dev.close()
        tail, _ = timed(lambda: bb.InsulationTrack(track.sums, track.counts, w, IGNORE, n, RES))
        say("    window %-4d kernel with the index built %s; the first call, with the index build, "
            "%.1f ms, of which the host tail %.1f ms; the dense route's bits: %s"
            % (w, spread(ms), first * 1e3, tail * 1e3, same))


if __name__ == "__main__":
    args = sys.argv[1:]
    main(int(args[0]) if args else 24927, int(args[1]) if len(args) > 1 else 11)
