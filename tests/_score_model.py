"""Float64 model of SPEC 2.8 (bb_solver_score / StructureSolver.score) in numpy.  Test-only.

score_sums(wish, x) gives the two arrays the device forms -- (n, 9) per genomic separation and
(n, 3) per bin -- over the pairs i < j with delta > 0, every term computed as SPEC 2.8 writes
it (products and sums rounded one by one, a correctly rounded root and quotients) and summed
in extended precision, so the model's own summation error is far below one float64 ulp of the
sum; on the exact inputs of exact_case() every term and every sum is a multiple of 1/64 below
2^53 and the model is exact."""
import numpy

from tests._engines import OracleEngine

WISH_FLOOR = {"float32": 1e-30, "float64": 1e-290}        # SPEC 2.1
WISH_CEILING = {"float32": float(numpy.finfo(numpy.float32).max),
                "float64": float(numpy.finfo(numpy.float64).max)}     # SPEC 2.1


def stored_wish(wish, dtype="float64"):
    """The delta the units hold for a kind='wish' input, widened to float64: the upper triangle,
    0 = no constraint for anything not finite, not positive, below the wish floor or above
    the largest finite value of the run's dtype (both compared in float64), then rounded to
    that dtype."""
    w = numpy.triu(numpy.asarray(wish, dtype=numpy.float64), 1)
    w = numpy.where(numpy.isfinite(w) & (w >= WISH_FLOOR[dtype]) & (w <= WISH_CEILING[dtype]), w, 0.0)
    return w.astype(dtype).astype(numpy.float64)


def _segment_sums(values, keys, n):
    """out[q] = the sum of values[keys == q] for q < n, keys ascending, in extended precision."""
    counts = numpy.bincount(keys, minlength=n)
    starts = numpy.concatenate([[0], numpy.cumsum(counts)[:-1]])
    out = numpy.zeros(n)
    if len(values):
        full = counts > 0
        out[full] = numpy.add.reduceat(values.astype(numpy.longdouble), starts[full]).astype(numpy.float64)
    return out


def score_sums(wish, x, mask=None, dtype="float64", with_magnitudes=False):
    """(profile (n, 9), bins (n, 3)) of SPEC 2.8.  mask: (n, n) bool, the pairs to take (a
    rank's own).  with_magnitudes: also the same two arrays with (d + delta) in place of
    (d - delta) -- the magnitudes B the error bound of a residual column is stated in (the
    columns without a residual are their own B)."""
    w = stored_wish(wish, dtype)
    x = numpy.asarray(x, dtype=numpy.float64)
    n = w.shape[0]
    on = w > 0
    if mask is not None:
        on &= numpy.asarray(mask, dtype=bool)
    i, j = numpy.nonzero(on)                           # the pairs, i < j, ordered by (i, j)
    delta = w[i, j]
    dx, dy, dz = (x[i, c] - x[j, c] for c in range(3))
    d = numpy.sqrt((dx * dx + dy * dy) + dz * dz)
    k = j - i
    key = numpy.int16 if n < 2 ** 15 else numpy.int64      # (16-bit keys sort by radix: 10x faster)
    by_k, by_j = numpy.argsort(k.astype(key), kind="stable"), numpy.argsort(j.astype(key), kind="stable")
    k_sorted, j_sorted = k[by_k], j[by_j]

    def residual_terms(res):
        u = res / delta
        return [res * res, (res * res) / delta, u * u]

    def sums(terms, cols, bin_cols):
        profile, bins = numpy.zeros((n, 9)), numpy.zeros((n, 3))
        for col, t in zip(cols, terms):
            profile[:, col] = _segment_sums(t[by_k], k_sorted, n)
            if col in bin_cols:
                # (the halves of a bin's sum are each good to 2^-64: their float64 sum to 2^-53)
                bins[:, bin_cols.index(col)] = _segment_sums(t, i, n) + _segment_sums(t[by_j], j_sorted, n)
        return profile, bins

    plain = [numpy.ones_like(d), d, delta, d * d, delta * delta, d * delta]
    profile, bins = sums(plain + residual_terms(d - delta), range(9), (0, 6, 8))
    if not with_magnitudes:
        return profile, bins
    mag_profile, mag_bins = sums(residual_terms(d + delta), (6, 7, 8), (0, 6, 8))
    mag_profile[:, :6], mag_bins[:, 0] = profile[:, :6], bins[:, 0]
    return profile, bins, mag_profile, mag_bins


def derive(profile, bins):
    """The report FitScore derives, straight from the definitions."""
    tot = profile.sum(axis=0)
    n, sd, sw, sdd, sww, sdw = tot[:6]
    out = {"n_pairs": int(n), "stress": tot[6:9], "normalized_stress": tot[6] / sww if sww > 0 else numpy.nan}
    cov, vd, vw = sdw / max(n, 1) - sd * sw / max(n, 1) ** 2, sdd / max(n, 1) - (sd / max(n, 1)) ** 2, \
        sww / max(n, 1) - (sw / max(n, 1)) ** 2
    out["pearson"] = cov / numpy.sqrt(vd * vw) if n >= 2 and vd > 0 and vw > 0 else numpy.nan
    cnt = profile[:, 0]
    with numpy.errstate(invalid="ignore", divide="ignore"):
        out["pairs"] = cnt.astype(numpy.int64)
        out["mean_distance"] = numpy.where(cnt > 0, profile[:, 1] / cnt, numpy.nan)
        out["mean_wish"] = numpy.where(cnt > 0, profile[:, 2] / cnt, numpy.nan)
        out["rms_relative_error"] = numpy.where(cnt > 0, numpy.sqrt(profile[:, 8] / cnt), numpy.nan)
        out["bin_pairs"] = bins[:, 0].astype(numpy.int64)
        out["bin_stress"] = bins[:, 1]
        out["bin_relative"] = numpy.where(bins[:, 0] > 0, numpy.sqrt(bins[:, 2] / bins[:, 0]), numpy.nan)
    return out


def exact_case(n, seed=0):
    """(wish, x) on which every term of SPEC 2.8 and every sum is exact in float64 whatever the
    order: bins on a line at integer x in [0, 2048) (y = z = 0), delta in {1, 2, 4, 8}, about
    30 % of the pairs absent, a few bins without any pair and a few coincident bins.  Every term
    is a multiple of 1/64 and every sum stays below 2^48 of those up to n = 4,097."""
    rng = numpy.random.default_rng(1000 + 7 * n + seed)
    x = numpy.zeros((n, 3))
    x[:, 0] = rng.integers(0, 2048, n)
    if n >= 4:
        twins = rng.choice(n, size=max(2, min(n // 50, 12)) // 2 * 2, replace=False)
        x[twins[1::2], 0] = x[twins[0::2], 0]                    # coincident bins: d = 0
    w = numpy.exp2(rng.integers(0, 4, (n, n))).astype(numpy.float64)
    w[rng.random((n, n)) < 0.3] = 0.0
    w = numpy.triu(w, 1)
    if n >= 8:
        lonely = rng.choice(n, size=max(1, min(n // 100, 5)), replace=False)
        w[lonely, :] = 0.0
        w[:, lonely] = 0.0
    return w + w.T, x


def float_case(n, seed=0):
    """(wish, structure): the distances of a random walk with a third of the pairs dropped, and
    the walk plus noise, so that no residual vanishes."""
    from tests import _oracle
    xs = _oracle.random_walk(n, seed=seed)
    w = numpy.triu(_oracle.wish_from_coords(xs), 1)
    w[numpy.random.default_rng(50 + seed).random((n, n)) < 1.0 / 3.0] = 0.0
    return w + w.T, _oracle.noisy_init(xs)


def sums_and_bounds(wish, x, dtype="float64", mask=None, extra=0.0):
    """(profile, bins, profile_bound, bins_bound): the model and the |device - model| allowed per
    entry, (n + 16) 2^-53 B -- n the pairs in that sum, B the same sum with (d + delta) for
    (d - delta) (B = the sum itself for the columns without a residual): each term is within
    8 * 2^-53 of its B-term on either side, and a float64 sum of n non-negative terms in any
    order within n * 2^-53.  extra: added as extra * B (the kind='counts' allowance)."""
    p, b, mp, mb = score_sums(wish, x, mask=mask, dtype=dtype, with_magnitudes=True)
    return p, b, ((p[:, :1] + 16) * 2.0 ** -53 + extra) * mp, ((b[:, :1] + 16) * 2.0 ** -53 + extra) * mb


class ScoringOracleEngine(OracleEngine):
    """OracleEngine with bb_solver_score played by the model over this rank's own pairs."""

    def score(self, xyz=None):
        x = self.X if xyz is None else numpy.asarray(xyz, dtype=numpy.float64)
        return score_sums(self.w, x, mask=self._own_pairs(), dtype=self.dtype)
