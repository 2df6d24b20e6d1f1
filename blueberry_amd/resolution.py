"""A structure between two resolutions (docs/SPEC.md 2.12): host numpy, O(N), float64.

The bins are those of the pooled map: coarse bin I holds the fine bins
[I factor, min((I + 1) factor, n_bins)).  `coarsen_structure` takes a fine structure to the coarse
bins' means -- what `compare_structures` needs to set a fine fit beside a coarse one --
and `prolong_structure` lays a coarse structure out over the fine bins by linear interpolation:
a hand-made `init=` array.  Neither scales anything: the unit of length is the caller's."""
import numpy


def check_factor(factor):
    """`factor` as an int >= 1; a bool, a float or anything else is a ValueError."""
    if isinstance(factor, bool) or not isinstance(factor, (int, numpy.integer)) or int(factor) < 1:
        raise ValueError("factor must be an int >= 1")
    return int(factor)


def _structure(X):
    X = numpy.asarray(X, dtype=numpy.float64)
    if X.ndim != 2 or X.shape[1] != 3:
        raise ValueError("a structure must have shape (n, 3)")
    return X


def coarsen_structure(X, factor):
    """The (ceil(n / factor), 3) means of the rows of the (n, 3) structure `X` per coarse bin: the
    rows of a bin are added top to bottom and divided by their number.  A row with a non-finite
    coordinate is left out; a bin with no row left is NaN."""
    X, k = _structure(X), check_factor(factor)
    n = X.shape[0]
    nc = -(-n // k)
    padded = numpy.zeros((nc * k, 3))
    padded[:n] = X
    ok = numpy.zeros(nc * k, dtype=bool)
    ok[:n] = numpy.isfinite(X).all(axis=1)
    padded[~ok] = 0.0
    total, rows = numpy.zeros((nc, 3)), numpy.zeros(nc)
    for a in range(k):                       # top to bottom: fine row a of every bin at once
        total += padded[a::k]
        rows += ok[a::k]
    out = numpy.full((nc, 3), numpy.nan)
    some = rows > 0
    out[some] = total[some] / rows[some, None]
    return out


def prolong_structure(Xc, factor, n_bins):
    """The (n_bins, 3) structure that the coarse structure `Xc` -- ceil(n_bins / factor) rows --
    gives: every coordinate is `numpy.interp` at the fine bins 0 .. n_bins - 1 over the coarse
    bins' centres, (lo + hi - 1) / 2 of a bin [lo, hi) in fine-bin units; NaN rows of `Xc` are
    skipped, beyond the first and the last centre the end values hold.  No scaling.  No finite
    row: all NaN."""
    Xc, k = _structure(Xc), check_factor(factor)
    n = int(n_bins)
    if n < 0:
        raise ValueError("n_bins must not be negative")
    nc = -(-n // k)
    if Xc.shape[0] != nc:
        raise ValueError("Xc must have ceil(n_bins / factor) = %d rows, got %d" % (nc, Xc.shape[0]))
    lo = numpy.arange(nc, dtype=numpy.int64) * k
    hi = numpy.minimum(lo + k, n)
    centre = (lo + hi - 1) / 2.0
    ok = numpy.isfinite(Xc).all(axis=1)
    out = numpy.full((n, 3), numpy.nan)
    if ok.any() and n:
        fine = numpy.arange(n, dtype=numpy.float64)
        for c in range(3):
            out[:, c] = numpy.interp(fine, centre[ok], Xc[ok, c])
    return out
