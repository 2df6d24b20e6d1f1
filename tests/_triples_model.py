"""The reference of the triples-balancing tests (tests/test_triples_balance_cpu.py,
tests/test_gpu_triples_balance.py): a scipy.sparse / numpy float64 restatement of docs/SPEC.md
2.5.3 -- the matrix a triple list DEFINES (nan_to_num, binning, unordered pairs, the last triple
of a pair wins, bin n_bins never read), then 2.5.2 on it with `A @ x` for the products and
`numpy.bincount` for the diagonals -- and the triple lists those tests use.  Nothing here touches
the library under test.  Results that several tests need are computed once
(`functools.lru_cache`) and must be left unchanged by their users."""
import functools

import numpy
import scipy.sparse


# ---- the matrix the triples define ---------------------------------------------------------------
def upper_cells(triples, resolution, n_bins):
    """(i, j, value) with i <= j < n_bins, one entry per stored pair, sorted by (i, j): the last
    triple of a pair wins.  A bin outside [0, n_bins] raises ValueError; a pair that touches bin
    n_bins is dropped."""
    t = numpy.nan_to_num(numpy.asarray(triples, dtype=numpy.float64)).reshape(-1, 3)
    q = t[:, :2] / float(resolution)
    if not (numpy.abs(q) < 2147483648.0).all():
        raise ValueError("a position maps to a bin outside [0, n_bins]")
    b = q.astype(numpy.int64)                                  # (truncation, as the C cast)
    if b.size and (b.min() < 0 or b.max() > n_bins):
        raise ValueError("a position maps to a bin outside [0, n_bins]")
    keep = (b < n_bins).all(axis=1)
    b, v = b[keep], t[keep, 2]
    lo, hi = numpy.minimum(b[:, 0], b[:, 1]), numpy.maximum(b[:, 0], b[:, 1])
    key = lo * n_bins + hi
    # the first occurrence in the reversed list is the last in the list
    uniq, first = numpy.unique(key[::-1], return_index=True)
    v = v[::-1][first]
    return uniq // max(n_bins, 1), uniq % max(n_bins, 1), v


def symmetric_csr(i, j, v, n_bins, ignore_diags=0):
    """A of 2.5.2 as CSR: both directions of every counted pair, the band left out."""
    on = (j - i) >= ignore_diags
    i, j, v = i[on], j[on], v[on]
    off = i != j
    rows = numpy.concatenate([i, j[off]])
    cols = numpy.concatenate([j, i[off]])
    vals = numpy.concatenate([v, v[off]])
    return scipy.sparse.csr_matrix((vals, (rows, cols)), shape=(n_bins, n_bins))


def _mask(a, min_nnz):
    nnz = numpy.asarray((a != 0).sum(axis=1)).ravel()
    live = nnz >= min_nnz
    while True:
        now = live & ((a @ live.astype(numpy.float64)) > 0.0)
        if numpy.array_equal(now, live):
            return live
        live = now


def balance(triples, resolution, n_bins, ignore_diags=0, min_nnz=0, tol=1e-5, max_iter=200,
            row_sum=None):
    """2.5.3: a dict with bias (NaN at dead bins), masked, iterations, variance, converged, and
    variances (var of every evaluated iteration: iterations + 1 values)."""
    i, j, v = upper_cells(triples, resolution, n_bins)
    n_bad = int(((v < 0.0) & ((j - i) >= ignore_diags)).sum())
    if n_bad:
        raise ValueError("%d counted cells are negative" % n_bad)
    a = symmetric_csr(i, j, v, n_bins, ignore_diags)
    live = _mask(a, min_nnz)
    n_live = int(live.sum())
    if n_live == 0:
        raise ValueError("no live bin is left")
    b = numpy.ones(n_bins)
    x = live.astype(numpy.float64)
    it, mean0, variances = 0, None, []
    while True:
        s = (x * (a @ x))[live]
        mean = s.sum() / n_live
        var = ((s / mean - 1.0) ** 2).sum() / n_live
        variances.append(var)
        if mean0 is None:
            mean0 = mean
        if var < tol or it == max_iter:
            break
        b[live] *= s / mean
        x[live] = 1.0 / b[live]
        it += 1
    b *= numpy.sqrt(mean / (mean0 if row_sum is None else row_sum))
    b[~live] = numpy.nan
    return {"bias": b, "masked": ~live, "iterations": it, "variance": var, "converged": var < tol,
            "variances": variances}


def pair_counts(live):
    """counts[k] = #{i : live_i and live_{i+k}}, exact, from the DEAD bins (few): n - k, less the
    pairs with a dead first or second end, plus those with both."""
    n = live.shape[0]
    k = numpy.arange(n)
    dead = numpy.flatnonzero(~live)
    cum = numpy.concatenate([[0], numpy.cumsum(~live)])        # cum[m] = dead bins below m
    first = cum[n - k]                                         # dead i with i < n - k
    second = cum[n] - cum[k]                                   # dead i + k, i.e. dead bins >= k
    diff = (dead[None, :] - dead[:, None]).ravel()
    both = numpy.bincount(diff[diff >= 0], minlength=n)[:n]
    return ((n - k) - first - second + both).astype(numpy.int64)


def expected(triples, resolution, n_bins, bias=None):
    """(sums, counts, e) of 2.5.3."""
    i, j, v = upper_cells(triples, resolution, n_bins)
    if bias is None:
        x = numpy.ones(n_bins)
    else:
        bias = numpy.asarray(bias, dtype=numpy.float64)
        with numpy.errstate(divide="ignore"):
            x = numpy.where(numpy.isnan(bias), 0.0, 1.0 / bias)
    p = x[i] * x[j]
    on = p != 0.0
    sums = numpy.bincount((j - i)[on], weights=(v * p)[on], minlength=n_bins)[:n_bins]
    counts = pair_counts(x != 0.0)
    ok = (counts > 0) & (sums != 0.0)
    e = numpy.full(n_bins, numpy.nan)
    e[ok] = sums[ok] / counts[ok]
    return sums, counts, e


# ---- triple lists ----------------------------------------------------------------------------
RESOLUTION = 10000


def triples_of_matrix(m, resolution=RESOLUTION, border=True):
    """The non-zero cells of the upper triangle of the leading n_bins x n_bins block of the
    (n_bins + 1)^2 matrix `m`, row by row, as triples -- and (border) every cell of column
    n_bins, whatever it holds: pairs that touch bin n_bins, which nothing may read."""
    d = m.shape[0]
    n = d - 1
    a = numpy.triu(numpy.asarray(m, dtype=numpy.float64)[:n, :n])
    i, j = numpy.nonzero(a)
    rows = [numpy.column_stack([i * float(resolution), j * float(resolution), a[i, j]])]
    if border:
        r = numpy.arange(d)
        rows.append(numpy.column_stack([r * float(resolution), numpy.full(d, n * float(resolution)),
                                        numpy.asarray(m)[:, n]]))
    return numpy.ascontiguousarray(numpy.concatenate(rows))


@functools.lru_cache(maxsize=None)
def hic_like_triples(n_bins, seed=None, band=24, far_per_bin=1.0):
    """A duplicate-free Hi-C-like pixel list over n_bins bins, `numpy.random.default_rng(seed)`
    (seed None: n_bins): Poisson counts of 200 (1 + |i - j|)^-1.08 b_i b_j, b = exp(N(0, 0.4)),
    3 % dead bins (no triple names them), EVERY pair of live bins within `band` of the diagonal
    (a count of 0 included: a stored zero cell) plus far_per_bin n_bins random far pairs.
    Positions lie anywhere inside their bins.  READ-ONLY (shared)."""
    rng = numpy.random.default_rng(n_bins if seed is None else seed)
    n = n_bins
    b = numpy.exp(rng.normal(0.0, 0.4, size=n))
    dead = rng.random(n) < 0.03
    i = numpy.repeat(numpy.arange(n), band + 1)
    j = i + numpy.tile(numpy.arange(band + 1), n)
    n_far = int(far_per_bin * n)
    if n > band + 2 and n_far:
        fi = rng.integers(0, n, size=n_far)
        fj = rng.integers(0, n, size=n_far)
        lo, hi = numpy.minimum(fi, fj), numpy.maximum(fi, fj)
        far = numpy.unique(lo[hi - lo > band] * n + hi[hi - lo > band])
        i = numpy.concatenate([i, far // n])
        j = numpy.concatenate([j, far % n])
    ok = (j < n) & ~dead[i] & ~dead[numpy.minimum(j, n - 1)]
    i, j = i[ok], j[ok]
    c = rng.poisson(200.0 * (1.0 + (j - i)) ** -1.08 * b[i] * b[j]).astype(numpy.float64)
    order = rng.permutation(i.shape[0])                        # (a file is in no particular order)
    i, j, c = i[order], j[order], c[order]
    flip = rng.random(i.shape[0]) < 0.5                        # ... and in either orientation
    pi = numpy.where(flip, j, i) * float(RESOLUTION) + rng.integers(0, RESOLUTION, size=i.shape[0])
    pj = numpy.where(flip, i, j) * float(RESOLUTION) + rng.integers(0, RESOLUTION, size=i.shape[0])
    t = numpy.ascontiguousarray(numpy.column_stack([pi, pj, c]))
    t.flags.writeable = False
    return t


@functools.lru_cache(maxsize=None)
def hic_like_triples_balance(n_bins, ignore_diags, min_nnz, tol, max_iter):
    """The model's result on hic_like_triples(n_bins).  READ-ONLY (shared)."""
    return balance(hic_like_triples(n_bins), RESOLUTION, n_bins, ignore_diags, min_nnz, tol, max_iter)
