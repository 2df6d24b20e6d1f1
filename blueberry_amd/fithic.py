"""Fit-Hi-C significance of a raw map on the device (docs/SPEC.md 2.9): a p-value and a q-value
for every stored contact of one chromosome.

The counterpart of the reference's `FitHiC(...).fit_transform(...)` (`blueberry/fithic.py`), which
reads three gzipped text files and writes a fourth, one line at a time.  Here the map is a
resident `ContactMap` or `DeviceTriples`: the per-distance tallies come from the sweep `expected`
already has, the equal-occupancy binning, the spline and the isotonic fit are O(n_bins) host work
in float64, and the pass over the in-range upper triangle -- the list of stored cells in canonical
order and the binomial survival function of each -- runs on the device (`bb_cm_significance`,
`bb_triples_significance`).  The result is a `FithicContactMap`, so `decimate`, `contacts`,
`to_matrix` and `to_sparse` (into `StructureSolver.fit`) work on it as they are.

Deviations from the reference, all deliberate: one range rule, `min_dist < distance
<= max_dist`, everywhere; the q-value column is filled in (Benjamini-Hochberg over the listed
p-values with the number of possible in-range pairs as the number of tests); `n_passes` is accepted
and unused, as in the reference, where only the first pass runs.
"""
import numpy

from . import _lib
from .datatypes import ContactMap, FithicContactMap, expected_sums
from .ranks import pick_device, several_ranks

_DIST_SCALING = 10000.0            # `distScaling`, blueberry/fithic.py:45


def binomial_sf(k, n, p, device=None):
    """P(X >= k) for X ~ Binomial(n, p), elementwise over `k` and `p` (broadcast together) for one
    whole number `n`, in float64 on the device (`bb_binomial_sf`): Loader's saddle-point pmf at the
    first term and the ratio recurrence of the tail.  Within 1.2e-13 of an 80-digit sum
    over the truth table on which `scipy.special.bdtrc(k - 1, n, p)` is off by up to 1.7e-3
    (docs/MEASUREMENTS.md).  k <= 0 gives 1,
    k > n gives 0, p outside [0, 1] gives NaN.  ValueError if some 0 < p < 1 has n * p above
    1,048,576."""
    k = numpy.asarray(k)
    if k.dtype.kind not in "iu":
        if not numpy.all(numpy.isfinite(k) & (k == numpy.floor(k)) & (numpy.abs(k) < 2.0 ** 63)):
            raise ValueError("binomial_sf: k must hold whole numbers of the int64 range")
    k, p = numpy.broadcast_arrays(k.astype(numpy.int64), numpy.asarray(p, dtype=numpy.float64))
    shape = k.shape
    k = numpy.ascontiguousarray(k).reshape(-1)
    p = numpy.ascontiguousarray(p).reshape(-1)
    n = float(n)
    if not (n >= 0.0 and n <= 2.0 ** 53 and n == numpy.floor(n)):
        raise ValueError("binomial_sf: n must be a whole number in [0, 2^53]")
    out = numpy.empty(k.shape[0], dtype=numpy.float64)
    _lib.check(_lib.load().bb_binomial_sf(k.ctypes.data_as(_lib.p_i64), n, _lib.as_f64_ptr(p),
                                          _lib.as_f64_ptr(out), k.shape[0],
                                          pick_device(device, several_ranks())),
               "bb_binomial_sf")
    return out.reshape(shape)


# ---- the host steps, O(n_bins) in float64 ------------------------------------------------------
def in_range_diagonals(n, resolution, min_dist, max_dist):
    """(k_lo, k_hi): the diagonals k < n with min_dist < k * resolution <= max_dist
    (`blueberry/fithic.py:445-449`); k_lo > k_hi if there is none."""
    k_lo = int(min_dist) // int(resolution) + 1
    k_hi = min(int(n) - 1, int(max_dist) // int(resolution))
    return k_lo, k_hi


def equal_occupancy(possible, observed, k_lo, k_hi, resolution, n_bins):
    """The equal-occupancy binning of the in-range diagonals (`blueberry/fithic.py:160-227`):
    (x, y), per bin the pair-weighted mean distance and the mean contact probability of a pair.
    A bin closes with the diagonal that fills it; what is left over at the end is dropped."""
    total = float(observed[k_lo:k_hi + 1].sum())
    desired = float(int(total) // int(n_bins))        # (the reference's integer division)
    x, y = [], []
    first, seen, acc, closed = k_lo, 0.0, 0.0, 0
    for k in range(k_lo, k_hi + 1):
        o = float(observed[k])
        seen += o
        if o >= desired or acc + o >= desired:
            closed += 1
            if closed < n_bins:
                desired = 1.0 * (total - seen) / (n_bins - closed)
            pairs = reads = dist = 0.0
            for b in range(first, k + 1):             # (in the reference's order of additions)
                pairs += possible[b]
                reads += observed[b]
                dist += 1.0 * possible[b] * (b * resolution / _DIST_SCALING)
            y.append((reads / pairs) / total)
            x.append(_DIST_SCALING * (dist / pairs))
            first, acc = k + 1, 0.0
        else:
            acc += o
    return numpy.array(x, dtype=numpy.float64), numpy.array(y, dtype=numpy.float64)


def isotonic_nonincreasing(y):
    """The least-squares non-increasing fit of `y` with unit weights: pool adjacent violators
    (what `IsotonicRegression(increasing=False)` computes at `blueberry/fithic.py:361-362`)."""
    y = numpy.asarray(y, dtype=numpy.float64)
    sums = numpy.empty(y.shape[0])
    lens = numpy.empty(y.shape[0], dtype=numpy.int64)
    top = 0
    for v in y:
        sums[top], lens[top] = v, 1
        top += 1
        # a block whose mean exceeds its predecessor's is pooled with it
        while top > 1 and sums[top - 2] * lens[top - 1] < sums[top - 1] * lens[top - 2]:
            sums[top - 2] += sums[top - 1]
            lens[top - 2] += lens[top - 1]
            top -= 1
    return numpy.repeat(sums[:top] / lens[:top], lens[:top])


def prior_by_distance(x, y, n, resolution, k_lo, k_hi):
    """(spline_x, spline_y, f): scipy's smoothing spline through the binning points with
    s = min(y)^2, evaluated at the in-range distances inside [min x, max x], made non-increasing
    (`blueberry/fithic.py:339-362`); and the lookup of `:429-430` as a table f[k], k = 0 .. n - 1:
    k * resolution clamped to [min x, max x], bisect_left, capped at the last index."""
    from scipy.interpolate import UnivariateSpline
    spline = UnivariateSpline(x, y, s=float(numpy.min(y)) ** 2)
    lo, hi = float(numpy.min(x)), float(numpy.max(x))
    dist = numpy.arange(k_lo, k_hi + 1, dtype=numpy.float64) * float(resolution)
    sx = dist[(dist >= lo) & (dist <= hi)]
    if sx.shape[0] == 0:
        raise ValueError("FitHiC: no in-range distance lies between the first and the last "
                         "binning point")
    sy = isotonic_nonincreasing(spline(sx))
    at = numpy.clip(numpy.arange(int(n), dtype=numpy.float64) * float(resolution), lo, hi)
    f = sy[numpy.minimum(numpy.searchsorted(sx, at, side="left"), sx.shape[0] - 1)]
    return sx, sy, numpy.ascontiguousarray(f, dtype=numpy.float64)


class _Results(_lib.Handle):
    """Owner of one bb_sig handle, made by a significance pass or by `select`."""
    prefix = "bb_sig_"

    def size(self):
        n, terms = _lib.c_i64(), _lib.c_i64()
        self._call("size", n, terms)
        return int(n.value), int(terms.value)

    def timing(self):
        a, b = _lib.c_dbl(), _lib.c_dbl()
        self._call("timing", a, b)
        return float(a.value), float(b.value)

    def read(self):
        m = self.size()[0]
        row, col = numpy.empty(m, dtype=numpy.int32), numpy.empty(m, dtype=numpy.int32)
        count, p = numpy.empty(m, dtype=numpy.float64), numpy.empty(m, dtype=numpy.float64)
        self._call("read", row.ctypes.data_as(_lib.p_i32), col.ctypes.data_as(_lib.p_i32),
                   _lib.as_f64_ptr(count), _lib.as_f64_ptr(p))
        return row, col, count, p

    def q_values(self, n_tests):
        """Compute the q-values of the resident p-values with `n_tests` tests and keep them on the
        handle (`bb_sig_q_values`; again: recomputed).  Returns the HIP-event times (ms) of keys +
        sort and of gather + scan + scatter."""
        a, b = _lib.c_dbl(), _lib.c_dbl()
        self._call("q_values", int(n_tests), a, b)
        return float(a.value), float(b.value)

    def read_q(self):
        """The q-values, in list order; RuntimeError before `q_values`."""
        q = numpy.empty(self.size()[0], dtype=numpy.float64)
        self._call("read_q", _lib.as_f64_ptr(q))
        return q

    def select(self, q_max):
        """The cells with q <= `q_max` as a new `_Results` (close it), in list order; a NaN q is
        never selected.  RuntimeError before `q_values`, ValueError for a NaN `q_max`."""
        out = _lib.c_void_p()
        self._call("select", float(q_max), out)
        return _Results(out)


def diagonal_sums(X, n):
    """O_k = sum_i M[i, i + k], k = 0 .. n - 1, of the map's leading n x n block: the sweep of
    `expected` with all weights 1 (`bb_cm_expected` / `bb_triples_expected`, bias NULL).  Leaves
    the map's own expected vector alone."""
    return expected_sums(X._balance_target(), n)[0]


def significance_list(X, n, k_lo, k_hi, bias, bias_range, prior, n_reads):
    """The device pass: the listed cells of the map in canonical order and their p-values, as a
    `_Results` (close it).  `bias`, `prior`: n float64 values each."""
    lo, hi = (-numpy.inf, numpy.inf) if bias_range is None else bias_range
    out = _lib.c_void_p()
    X._balance_target()._call("significance", int(n), int(k_lo), int(k_hi), _lib.as_f64_ptr(bias),
                              float(lo), float(hi), _lib.as_f64_ptr(prior), float(n_reads), out)
    return _Results(out)


class FitHiC(object):
    """Fit-Hi-C (Ay, Bailey and Noble 2014) at the level of a map's bins, for one chromosome.

    Parameters (the order and defaults of `blueberry/fithic.py:76-83`)
    ----------
    libname : str, optional
        Kept for the signature; nothing is written.
    resolution : int
        The bin size of the map.
    n_bins : int, optional
        The number of equal-occupancy bins.  Default is 100.
    n_passes : int, optional
        Accepted and unused: the reference runs the first pass only.
    max_dist, min_dist : int, optional
        A pair at distance d is in range iff min_dist < d <= max_dist.  -1: 10,000,000 and 0.
    bias_range : (low, high) or None
        A bin whose bias lies outside is not tested (`blueberry/fithic.py:147`); None: no bounds.

    After `fit_transform`: `bins_x_`, `bins_y_` (the binning points), `spline_x_`, `spline_y_` (the
    non-increasing spline), `prior_by_distance_` (its lookup table per diagonal), `n_reads_` (N: the
    in-range reads), `n_tests_` (T: the possible in-range pairs), `n_listed_` (the contacts listed);
    `terms_` (pmf values the device summed), `list_ms_` and `p_ms_` (HIP-event times of the call's
    two device passes), `sort_ms_` and `bh_ms_` (those of the q-values: keys and sort; gather, scan
    and scatter), `n_selected_` (the contacts returned: `n_listed_` without `q_max`).
    """

    def __init__(self, libname=None, resolution=None, n_bins=100, n_passes=2, max_dist=-1,
                 min_dist=-1, bias_range=(0.5, 2.0)):
        if resolution is None or int(resolution) < 1:
            raise ValueError("FitHiC: resolution must be a positive integer")
        if int(n_bins) < 1:
            raise ValueError("FitHiC: n_bins must be at least 1")
        if (max_dist != -1 and max_dist < 0) or (min_dist != -1 and min_dist < 0):
            raise ValueError("FitHiC: min_dist and max_dist must not be negative (-1: the default)")
        self.libname = libname
        self.resolution = int(resolution)
        self.n_bins = int(n_bins)
        self.n_passes = n_passes
        self.max_dist = int(max_dist) if max_dist != -1 else 10000000
        self.min_dist = int(min_dist) if min_dist != -1 else 0
        if self.min_dist >= self.max_dist:
            raise ValueError("FitHiC: min_dist must be below max_dist")
        if bias_range is not None:
            lo, hi = (float(v) for v in bias_range)
            if not lo <= hi:
                raise ValueError("FitHiC: bias_range must be (low, high) with low <= high")
            bias_range = (lo, hi)
        self.bias_range = bias_range

    def _arguments(self, X, biases, map_bins):
        """(n, bias vector, k_lo, k_hi), every argument checked; no device call."""
        if isinstance(X, ContactMap):
            if map_bins is not None and int(map_bins) != X.n_bins:
                raise ValueError("FitHiC: map_bins does not match the map's n_bins")
            n, own = X.n_bins, X._KRnorm
        elif getattr(X, "is_triples", False):
            if map_bins is None:
                raise ValueError("FitHiC: a DeviceTriples needs map_bins")
            n, own = int(map_bins), None
        else:
            raise ValueError("FitHiC: X must be a ContactMap or a DeviceTriples")
        if int(X.resolution) != self.resolution:
            raise ValueError("FitHiC: the map's resolution is %d, not %d"
                             % (int(X.resolution), self.resolution))
        if n < 1:
            raise ValueError("FitHiC: the map has no bins")
        if isinstance(biases, str):
            if biases != "auto":
                raise ValueError("biases must be 'auto', None or a vector of n_bins values")
            biases = own
            if biases is not None:
                if biases.shape[0] < n:
                    raise ValueError("KRnorm shorter than n_bins")
                biases = biases[:n]
        if biases is None:
            bias = numpy.ones(n, dtype=numpy.float64)
        else:
            bias = numpy.ascontiguousarray(biases, dtype=numpy.float64)
            if bias.shape != (n,):
                raise ValueError("biases must have n_bins = %d values, got shape %r" % (n, bias.shape))
        k_lo, k_hi = in_range_diagonals(n, self.resolution, self.min_dist, self.max_dist)
        if k_lo > k_hi:
            raise ValueError("FitHiC: no diagonal of the map lies in the range (%d, %d]"
                             % (self.min_dist, self.max_dist))
        return n, bias, k_lo, k_hi

    def fit_transform(self, X, biases="auto", map_bins=None, q_max=None):
        """The p- and q-values of `X`'s contacts, as a `FithicContactMap` with rows (mid1, mid2,
        count, p, q), mid = bin * resolution + resolution // 2, in canonical order (row-major over
        i <= j).  The q-values are made on the device from the resident p-values
        (`bb_sig_q_values`, docs/SPEC.md 2.9.7).

        q_max : None -- every listed contact; a number -- only the contacts with q <= q_max (e.g.
            `Q_LOWER_BOUND`), selected on the device, so that only they are read back: the rows
            of the full result with `map[:, 4] <= q_max`, bit for bit and in order.

        X : a `ContactMap` holding raw counts, or a `DeviceTriples` together with `map_bins` (the
            n_bins of the map the triples define).  One chromosome.
        biases : 'auto' -- the map's KRnorm (what `balance()` left) if it has one, else all ones;
            None -- all ones; or a vector of n_bins values, NaN marking a dead bin.

        A counted cell that is negative, not finite or not a whole number raises ValueError
        ("significance needs raw counts"), found and counted on the device: by the list's counting
        pass, which a diagonal sum that is itself no count brings forward.  The map stays as it
        is."""
        n, bias, k_lo, k_hi = self._arguments(X, biases, map_bins)
        if q_max is not None:
            q_max = float(q_max)
            if q_max != q_max:
                raise ValueError("FitHiC: q_max is NaN")
        r = self.resolution
        observed = diagonal_sums(X, n)
        observed[:k_lo] = 0.0
        observed[k_hi + 1:] = 0.0
        possible = (n - numpy.arange(n)).astype(numpy.float64)
        n_reads = float(observed.sum())
        if not (numpy.isfinite(n_reads) and numpy.all(observed >= 0.0)
                and numpy.all(observed == numpy.floor(observed))):
            # the sums cannot be binned; the device's counting pass names the cells (it raises)
            significance_list(X, n, k_lo, k_hi, bias, None, numpy.zeros(n), 0.0).close()
            raise ValueError("FitHiC: significance needs raw counts: a diagonal sum is negative, "
                             "not finite or not a whole number")
        if n_reads > 2.0 ** 53:
            raise ValueError("FitHiC: more than 2^53 reads")
        n_tests = int(possible[k_lo:k_hi + 1].sum())
        x, y = equal_occupancy(possible, observed, k_lo, k_hi, r, self.n_bins)
        if x.shape[0] < 4:
            raise ValueError("FitHiC: the binning gave %d points; the spline needs at least 4 "
                             "(fewer reads than bins, or too narrow a range?)" % x.shape[0])
        sx, sy, prior = prior_by_distance(x, y, n, r, k_lo, k_hi)
        res = significance_list(X, n, k_lo, k_hi, bias, self.bias_range, prior, n_reads)
        picked = None
        try:
            (n_listed, self.terms_), (self.list_ms_, self.p_ms_) = res.size(), res.timing()
            self.sort_ms_, self.bh_ms_ = res.q_values(n_tests)
            if q_max is not None:
                picked = res.select(q_max)
            source = res if picked is None else picked
            row, col, count, p = source.read()
            q = source.read_q()
        finally:
            if picked is not None:
                picked.close()
            res.close()
        self.bins_x_, self.bins_y_, self.spline_x_, self.spline_y_ = x, y, sx, sy
        self.prior_by_distance_ = prior
        self.n_reads_, self.n_tests_, self.n_listed_ = n_reads, n_tests, n_listed
        self.n_selected_ = int(p.shape[0])
        mids = numpy.column_stack([row, col]).astype(numpy.float64) * r + r // 2
        return FithicContactMap.from_array(
            numpy.column_stack([mids, count, p, q]).reshape(-1, 5), r,
            celltype=getattr(X, "celltype", ""), chromosome=getattr(X, "chromosome", 0))


def _significance(X, map_bins, kwargs):
    """`ContactMap.significance` / `DeviceTriples.significance`: FitHiC's constructor arguments and
    `biases` and `q_max` as keywords; the map's own resolution."""
    kwargs = dict(kwargs)
    biases = kwargs.pop("biases", "auto")
    q_max = kwargs.pop("q_max", None)
    kwargs.setdefault("resolution", X.resolution)
    return FitHiC(**kwargs).fit_transform(X, biases=biases, map_bins=map_bins, q_max=q_max)
