"""Cost of pooling a map to a coarser resolution (docs/SPEC.md 2.12) on the
Hi-C-like map of tests/_balance_model.hic_like_raw, by default d = 24,927 (chr1 at 10 kb):

  * dense (`bb_cm_coarsen`): the pooling kernel by HIP events (`bb_cm_coarsen_timing`), one warm
    call and the median (min..max) of `reps` calls, for factor 2, 5 and 10; the bytes are
    8 n (n + 1) / 2 read plus 8 (nc + 1)^2 written; the rate is put beside the stream-read figure
    of `HipEngine.stream_read_ms` measured in the same process;
  * pixel list (`bb_triples_coarsen`): the map's non-zero cells as triples; count + scan + write
    by HIP events with the index already on the handle (`bb_triples_coarsen_timing`), the
    synchronised wall clock of the whole call with the index built, and of the first call on a
    fresh handle, which builds the index.

    python tools/coarsen_timing.py [d] [reps]

Not a test; bench.py does not call it."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy  # noqa: E402

import blueberry_amd as bb  # noqa: E402
from blueberry_amd import _lib  # noqa: E402
from tests import _balance_model as bm  # noqa: E402
from tests import _triples_model as tm  # noqa: E402

RES = 10000
FACTORS = (2, 5, 10)


def say(line):
    print(line, flush=True)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()                                             # every call here ends synchronised
    return time.perf_counter() - t0, out


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


def spread(ms):
    return "%.4f ms (min %.4f max %.4f, %d calls)" % (statistics.median(ms), min(ms), max(ms), len(ms))


def main(d, reps):
    n = d - 1
    rate = stream_read_rate()
    say("stream read (HipEngine.stream_read_ms, fp32 units of 16,384 bins): %.3f TB/s" % (rate / 1e12))
    m = bm.hic_like_raw(d)
    t = tm.triples_of_matrix(m, RES, border=False)
    cmap = bb.ContactMap.from_matrix(m, resolution=RES)
    src = cmap._resident()
    del m
    say("dense, d = %d (%.2f GB resident):" % (d, d * d * 8 / 1e9))
    for k in FACTORS:
        nc = -(-n // k)
        dst = bb.datatypes._DeviceMatrix(nc + 1, src.device)
        ms = []
        for call in range(reps + 1):
            src._call("coarsen", n, k, _lib.BB_COARSEN_SUM, dst._open())
            ms.append(dst._get(_lib.c_dbl, "coarsen_timing"))
        dst.close()
        ms = ms[1:]
        nbytes = 8.0 * n * (n + 1) / 2 + 8.0 * (nc + 1) ** 2
        got = nbytes / (statistics.median(ms) * 1e-3)
        say("    factor %-3d nc = %-6d %s: %.1f MB = %.3f TB/s = %.3f of the stream read"
            % (k, nc, spread(ms), nbytes / 1e6, got / 1e12, got / rate))
    src.close()                                            # (the dense matrix leaves the device)
    del cmap
    say("pixel list, %d triples (%.2f GB):" % (t.shape[0], t.nbytes / 1e9))
    for k in FACTORS:
        dev = bb.DeviceTriples(t, RES, 0)
        first, pooled = timed(lambda: dev.coarsen(n, k))
        cells = pooled.n
        pooled.close()
        wall, ev = [], []
        for call in range(reps):
            w, pooled = timed(lambda: dev.coarsen(n, k))
            wall.append(w * 1e3)
            ev.append(pooled._get(_lib.c_dbl, "coarsen_timing"))
            pooled.close()
        dev.close()
        say("    factor %-3d %d pooled cells; count + scan + write by events %s; the call with the "
            "index built %.3f ms (median wall clock); the first call, with the index build, %.1f ms"
            % (k, cells, spread(ev), statistics.median(wall), first * 1e3))


if __name__ == "__main__":
    args = sys.argv[1:]
    main(int(args[0]) if args else 24927, int(args[1]) if len(args) > 1 else 11)
