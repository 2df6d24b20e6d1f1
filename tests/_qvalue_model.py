"""A numpy model of the q-value rule's sort key (docs/SPEC.md 2.9.7) and the input families its
tests share.  No device, no package import."""
import numpy

TOP = numpy.uint64(1) << numpy.uint64(63)
ALL = numpy.uint64(0xFFFFFFFFFFFFFFFF)

# +-0, +-inf, +-NaN, the denormals next to zero, the smallest normals, and two ordinary values
SPECIALS = numpy.array([0.0, -0.0, numpy.inf, -numpy.inf, numpy.nan, -numpy.nan, 5e-324, -5e-324,
                        2.2250738585072014e-308, -2.2250738585072014e-308, 1.0, 0.5])

FAMILIES = ("bits", "specials", "equal", "uniform", "ulp", "sorted", "reversed")


def key(p):
    """The 64-bit key of every float64 of `p`: its unsigned order is numpy's sort order."""
    p = numpy.ascontiguousarray(p, dtype=numpy.float64)
    b = p.view(numpy.uint64)
    k = numpy.where((b & TOP) != 0, ~b, b | TOP)
    k = numpy.where(p == 0.0, TOP, k)
    return numpy.where(numpy.isnan(p), ALL, k)


def stable_order(p):
    """The stable sorted order of `p` by the key (numpy's own stable sort of the uint64 keys)."""
    return numpy.argsort(key(p), kind="stable")


def family(name, m, seed=0):
    """m float64 values of the family `name`."""
    rng = numpy.random.default_rng([seed, m, FAMILIES.index(name)])
    if name == "bits":            # every digit of all eight passes varies; NaNs and negatives
        return rng.integers(0, 2 ** 64, m, dtype=numpy.uint64).view(numpy.float64)
    if name == "specials":        # heavy ties
        return SPECIALS[rng.integers(0, SPECIALS.shape[0], m)]
    if name == "equal":
        return numpy.full(m, 0.3)
    if name == "ulp":             # 0.25 + j 2^-54, j < 256: only the lowest digit differs
        return 0.25 + rng.integers(0, 256, m) * 2.0 ** -54
    u = rng.random(m)
    if name == "uniform":
        return u
    return numpy.sort(u) if name == "sorted" else numpy.sort(u)[::-1].copy()
