#!/usr/bin/env python3
"""What the 24-bit stream of the fp32 sweep (docs/SPEC.md 3.7) covers on the benchmark's map: a
numpy model of the rule, no GPU.  For the seeded random walk at N bins it prints, for the
integer-offset code (max - min < 2^24 over a unit's words as uint32) and for comparison a code
that wants the top byte constant per unit: packable units, stream bytes with runs >= R only, and
format switches per wave.

    python tools/pack24_coverage.py [--bins 50000] [--seed 0] [--min-run 64] [--waves 2048]
"""
import argparse
import os
import sys

import numpy

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import _oracle  # noqa: E402

VW, RPU, UPT = 512, 4, 128


def unit_minmax(xs, n):
    """min and max word (uint32) of every unit of the dense fp32 layout, strip-major; also the
    smallest and largest top byte."""
    nb = -(-n // VW)
    pad = numpy.zeros((nb * VW, 3))
    pad[:n] = xs
    real = numpy.arange(nb * VW) < n
    lo, hi = [], []
    for J in range(nb):
        cj = pad[J * VW:(J + 1) * VW]
        for I in range(J + 1):
            ri = pad[I * VW:(I + 1) * VW]
            d = numpy.sqrt(((ri[:, None, :] - cj[None, :, :]) ** 2).sum(-1)).astype(numpy.float32)
            i = numpy.arange(I * VW, (I + 1) * VW)[:, None]
            j = numpy.arange(J * VW, (J + 1) * VW)[None, :]
            d[(i >= j) | ~real[i] | ~real[j]] = 0.0
            w = d.view(numpy.uint32).reshape(UPT, RPU * VW)
            lo.append(w.min(1))
            hi.append(w.max(1))
    return numpy.concatenate(lo).astype(numpy.int64), numpy.concatenate(hi).astype(numpy.int64)


def report(name, packable, min_run, waves):
    n = packable.size
    packed = numpy.zeros(n, dtype=bool)
    edges = numpy.flatnonzero(numpy.diff(packable.astype(numpy.int8))) + 1
    for a, b in zip(numpy.r_[0, edges], numpy.r_[edges, n]):
        packed[a:b] = packable[a] and b - a >= min_run
    q, r = divmod(n, waves)
    starts = numpy.arange(waves) * q + numpy.minimum(numpy.arange(waves), r)
    ends = starts + q + (numpy.arange(waves) < r)
    sw = numpy.array([int((packed[a + 1:b] != packed[a:b - 1]).sum()) for a, b in zip(starts, ends)])
    sw1 = numpy.array([int((packable[a + 1:b] != packable[a:b - 1]).sum()) for a, b in zip(starts, ends)])
    share = (6.0 * packed.sum() + 8.0 * (n - packed.sum())) / (8.0 * n)
    print("%-28s packable %5.1f %%  stream %.3f of raw (runs >= %d)  switches per wave mean %.2f max %d "
          "(no run rule: mean %.2f max %d)" % (name, 100.0 * packable.mean(), share, min_run, sw.mean(),
                                               sw.max(), sw1.mean(), sw1.max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bins", type=int, default=50000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--min-run", type=int, default=64)
    ap.add_argument("--waves", type=int, default=2048)
    a = ap.parse_args()
    xs = _oracle.random_walk(a.bins, seed=a.seed)
    lo, hi = unit_minmax(xs, a.bins)
    print("N = %d, %d units of %d x %d" % (a.bins, lo.size, RPU, VW))
    report("top byte constant per unit", (lo >> 24) == (hi >> 24), a.min_run, a.waves)
    report("integer offset, span < 2^24", hi - lo < (1 << 24), a.min_run, a.waves)


if __name__ == "__main__":
    main()
