#!/usr/bin/env python3
"""Writes tests/golden/binomial_sf_truth.npz: the multi-precision truth the binomial survival
function (docs/SPEC.md 2.9.6) is checked against, on the CPU and on the device.

Every row is (k, n, p, truth): truth = P(X >= k), X ~ Binomial(n, p), for the float64 p AS STORED,
summed with mpmath at 80 digits: the pmf from mp.loggamma at the first term, the exact ratio of
neighbouring pmf values from there, over the shorter side of k (the upper tail, or the lower tail
and its complement), until a term is below 1e-70 of the sum; then rounded to float64.
(mpmath.betainc does not converge for these arguments.)  Needs mpmath; runs for about a minute.

The rows: n from 1e2 to 3e9 x N p from 1e-6 to 3e3 x k in the body and both tails; the closed
cases; k on both sides of (n + 1) p; k = n; N p at the refusal limit 2^20.  Rows whose truth is
below 1e-290 are kept to under 5 % (the tests compare those for "result <= 1e-289" only)."""
import math
import os
import sys

import numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SF_MAX_MEAN = 1048576.0


def truth(k, n, p):
    import mpmath as mp
    mp.mp.dps = 80
    n_, p_ = mp.mpf(int(n)), mp.mpf(float(p))
    if k <= 0:
        return mp.mpf(1)
    if k > n:
        return mp.mpf(0)
    if p_ == 0:
        return mp.mpf(0)
    if p_ == 1:
        return mp.mpf(1)
    q_ = 1 - p_

    def pmf(x):
        x = mp.mpf(int(x))
        return mp.exp(mp.loggamma(n_ + 1) - mp.loggamma(x + 1) - mp.loggamma(n_ - x + 1)
                      + x * mp.log(p_) + (n_ - x) * mp.log1p(-p_))

    eps = mp.mpf(10) ** -70
    if k > (n + 1) * p_:
        j, term = int(k), pmf(k)
        total = term
        while j < n:
            term = term * (n_ - j) / (j + 1) * p_ / q_
            j += 1
            total += term
            if term < eps * total:
                break
        return total
    j, term = int(k) - 1, pmf(k - 1)
    total = term
    while j > 0:
        term = term * j / (n_ - j + 1) * q_ / p_
        j -= 1
        total += term
        if term < eps * total:
            break
    return 1 - total


def cases():
    rows = []

    def add(k, n, p):
        rows.append((int(k), float(n), float(p)))

    # the ranges: n x mean x k in the body and both tails
    for n in (1e2, 1e3, 1e4, 1e6, 1e8, 3e9):
        for mean in (1e-6, 1e-3, 0.1, 1.0, 10.0, 100.0, 3e3):
            if mean >= n:
                continue
            p = mean / n
            sd = math.sqrt(mean * (1 - p))
            ks = {2, 3, 5, math.floor(mean), math.floor(mean) + 1, math.ceil(mean - 6 * sd),
                  math.ceil(mean - 2 * sd), math.ceil(mean + 2 * sd), math.ceil(mean + 6 * sd),
                  math.ceil(mean + 12 * sd) + 3}
            for k in sorted(ks):
                if 2 <= k <= n:
                    add(k, n, p)
    # the closed cases
    for n in (1e2, 1e6, 3e9):
        body = 0.25 if n == 1e2 else 1e-4          # (n p stays below the refusal limit)
        for p in (1e-9, body):
            for k in (-3, 0, 1):
                add(k, n, p)
        for k in (0, 1, n):
            add(k, n, 1.0)
        add(n + 1, n, body)
        add(0, n, 0.0)
        add(1, n, 0.0)
    add(5, 1e2, 0.0)
    add(1e2, 1e2, 0.25)
    for n, p in ((1e2, 1e-3), (1e4, 1e-4), (1e6, 3e-6), (3e9, 1e-9), (3e9, 1e-15), (1e3, 0.5)):
        add(1, n, p)
    # k = n, and k on both sides of (n + 1) p
    for n, p in ((1e2, 0.5), (1e2, 0.99), (1e3, 0.9), (17.0, 0.3), (2.0, 0.5), (40.0, 0.999)):
        add(n, n, p)
        add(n - 1, n, p)
    for n, p in ((1e2, 0.5), (1e3, 0.0105), (1e6, 2.5e-4), (3e9, 1e-6), (99.0, 0.25), (1e4, 0.9)):
        edge = math.floor((n + 1) * p)
        for k in (edge - 1, edge, edge + 1, edge + 2):
            if k >= 2:
                add(k, n, p)
    # p above one half, where q is the small one
    for n, p in ((1e2, 0.9), (1e3, 0.75), (1e4, 0.999)):
        mean, sd = n * p, math.sqrt(n * p * (1 - p))
        for k in (math.ceil(mean - 8 * sd), math.ceil(mean - sd), math.ceil(mean + sd),
                  min(n, math.ceil(mean + 5 * sd))):
            add(k, n, p)
    # N p at the refusal limit
    for n, mean in ((2.0 ** 40, SF_MAX_MEAN), (3e9, SF_MAX_MEAN * (1 - 1e-9)), (2097152.0, SF_MAX_MEAN),
                    (1e8, 1e6)):
        p = mean / n
        while n * p > SF_MAX_MEAN:                 # the largest p the entry points accept
            p = math.nextafter(p, 0.0)
        sd = math.sqrt(mean * (1 - p))
        for k in (math.ceil(mean - 5 * sd), math.floor(mean), math.floor(mean) + 2,
                  math.ceil(mean + 3 * sd), math.ceil(mean + 8 * sd)):
            add(k, n, p)
    # far tails whose truth is below the float64 range (few)
    for k, n, p in ((400, 1e6, 1e-5), (900, 1e3, 1e-3), (100, 3e9, 1e-15), (5000, 1e4, 1e-2)):
        add(k, n, p)
    return sorted(set(rows), key=rows.index)


def main():
    rows = cases()
    k = numpy.array([r[0] for r in rows], dtype=numpy.int64)
    n = numpy.array([r[1] for r in rows], dtype=numpy.float64)
    p = numpy.array([r[2] for r in rows], dtype=numpy.float64)
    assert numpy.all((p == 0) | (p == 1) | (n * p <= SF_MAX_MEAN))
    t = numpy.array([float(truth(int(a), int(b), float(c))) for a, b, c in zip(k, n, p)])
    tiny = (t < 1e-290).mean()
    print("%d rows, %.1f %% below 1e-290, truth in [%.3g, %.3g]" % (t.size, 100 * tiny, t.min(), t.max()))
    assert tiny <= 0.05
    out = os.path.join(ROOT, "tests", "golden", "binomial_sf_truth.npz")
    numpy.savez_compressed(out, k=k, n=n, p=p, truth=t)
    print("wrote", out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
