"""The reference of the balancing tests (tests/test_balance_cpu.py, tests/test_gpu_balance.py): a
plain numpy float64 restatement of docs/SPEC.md 2.5.2 -- `A @ x` for the products, `numpy.trace(W,
k)` for the diagonals -- and the maps those tests use.  Nothing here touches the library under
test.  Results that several tests need are computed once (`functools.lru_cache`) and must be left
unchanged by their users."""
import functools

import numpy


# ---- the model -------------------------------------------------------------------------------
def counted_cells(m, ignore_diags=0):
    """A: the leading n_bins x n_bins block of the (n_bins + 1)^2 matrix `m`, symmetric from its
    UPPER triangle (the library reads nothing else), 0 inside the band |i - j| < ignore_diags."""
    from tests._large_maps import _add_transpose
    n = m.shape[0] - 1
    full = numpy.asarray(m, dtype=numpy.float64)[:n, :n]
    a = _add_transpose(numpy.triu(full, 1))                # (in cache-sized blocks)
    flat = a.reshape(-1)
    flat[::n + 1] = numpy.diagonal(full)
    # the band is SET to 0, not multiplied: a NaN or an infinity inside it is not counted either
    for k in range(min(ignore_diags, n)):
        flat[k::n + 1][:n - k] = 0.0
        flat[k * n::n + 1][:n - k] = 0.0
    return a


def offending_cells(m, ignore_diags=0):
    """The number of counted cells of the upper triangle that are negative or not finite."""
    n = m.shape[0] - 1
    a = numpy.asarray(m, dtype=numpy.float64)[:n, :n]
    i = numpy.arange(n)
    counted = (i[None, :] - i[:, None]) >= ignore_diags
    with numpy.errstate(invalid="ignore"):
        bad = ~(numpy.isfinite(a) & (a >= 0.0))
    return int((bad & counted).sum())


def balance_mask(a, min_nnz=0):
    """The live bins: at least min_nnz non-zero counted cells (raw map, once), then the fixed
    point of "the marginal over the cells shared with live bins is not 0"."""
    live = (a != 0).sum(axis=1) >= min_nnz
    while True:
        now = live & ((a @ live.astype(numpy.float64)) > 0.0)
        if numpy.array_equal(now, live):
            return live
        live = now


def balance(m, ignore_diags=0, min_nnz=0, tol=1e-5, max_iter=200, row_sum=None):
    """Iterative correction as docs/SPEC.md 2.5.2 states it.  Returns a dict: bias (NaN at dead
    bins), masked, iterations, variance, converged, and variances (var of every evaluated
    iteration: iterations + 1 values)."""
    if offending_cells(m, ignore_diags):
        raise ValueError("negative or non-finite counted cells")
    a = counted_cells(m, ignore_diags)
    n = a.shape[0]
    live = balance_mask(a, min_nnz)
    n_live = int(live.sum())
    if n_live == 0:
        raise ValueError("no live bin is left")
    b = numpy.ones(n)
    x = live.astype(numpy.float64)
    it, variances, mean0 = 0, [], None
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


def expected(m, bias=None):
    """(sums, counts, e) of docs/SPEC.md 2.5.2: sums[k] = sum_i M[i, i+k] x_i x_{i+k} over the
    pairs with x_i x_{i+k} != 0, counts[k] their number, x = 1 / bias (0 where it is NaN);
    e = sums / counts, NaN where counts == 0 or sums == 0."""
    n = m.shape[0] - 1
    a = numpy.asarray(m, dtype=numpy.float64)[:n, :n]
    if bias is None:
        x = numpy.ones(n)
    else:
        bias = numpy.asarray(bias, dtype=numpy.float64)
        with numpy.errstate(divide="ignore"):
            x = numpy.where(numpy.isnan(bias), 0.0, 1.0 / bias)
    p = x[:, None] * x[None, :]
    on = p != 0.0
    with numpy.errstate(invalid="ignore", over="ignore"):
        w = numpy.where(on, a * p, 0.0)
    sums = numpy.array([numpy.trace(w, k) for k in range(n)], dtype=numpy.float64).reshape(n)
    counts = numpy.array([numpy.trace(on, k, dtype=numpy.int64) for k in range(n)],
                         dtype=numpy.int64).reshape(n)
    ok = (counts > 0) & (sums != 0.0)
    e = numpy.full(n, numpy.nan)
    e[ok] = sums[ok] / counts[ok]
    return sums, counts, e


# ---- maps ------------------------------------------------------------------------------------
def circulant_planted(n, seed):
    """(matrix of n bins + the zero padding row, p, C): M_ij = p_i p_j C_{min(|i-j|, n-|i-j|)},
    C_k = 100 (1 + k)^-1.08, p = exp(N(0, 0.6)).  Every row of the circulant C has the same sum,
    so the balanced map is a multiple of C and the bias a multiple of p."""
    rng = numpy.random.default_rng(seed)
    p = numpy.exp(rng.normal(0.0, 0.6, size=n))
    i = numpy.arange(n)
    sep = numpy.abs(i[:, None] - i[None, :])
    ring = numpy.minimum(sep, n - sep)
    c = 100.0 * (1.0 + numpy.arange(n)) ** -1.08
    m = numpy.zeros((n + 1, n + 1))
    m[:n, :n] = p[:, None] * p[None, :] * c[ring]
    return m, p, c


@functools.lru_cache(maxsize=None)
def hic_like_raw(d, seed=None):
    """A raw Hi-C-like map of d - 1 bins (edge d): Poisson counts of 200 (1 + |i - j|)^-1.08
    bias_i bias_j with bias = exp(N(0, 0.4)) and 3 % dead bins, `numpy.random.default_rng(seed)`
    (seed None: d).  Row and column d - 1 are the zero padding.  READ-ONLY (shared)."""
    n = d - 1
    rng = numpy.random.default_rng(d if seed is None else seed)
    bias = numpy.exp(rng.normal(0.0, 0.4, size=n))
    bias[rng.random(n) < 0.03] = 0.0
    decay = 200.0 * (1.0 + numpy.arange(n)) ** -1.08
    m = numpy.zeros((d, d))
    for i in range(n):                                     # the upper triangle, a row at a time
        m[i, i:n] = rng.poisson(decay[:n - i] * (bias[i] * bias[i:n]))
    m[:n, :n] += numpy.triu(m[:n, :n], 1).T
    m.flags.writeable = False
    return m


@functools.lru_cache(maxsize=None)
def hic_like_balance(d, ignore_diags, min_nnz, tol, max_iter):
    """The model's result on hic_like_raw(d), or None where the model refuses the map (no live
    bin).  READ-ONLY (shared)."""
    try:
        return balance(hic_like_raw(d), ignore_diags, min_nnz, tol, max_iter)
    except ValueError:
        return None


# (d, ignore_diags, min_nnz) of every `tol=1e-5` run the device is asked for: the CPU test asserts
# that the model stops clear of tol on these, the GPU test that the device stops where it does
STOP_CASES = [(d, 2, 10) for d in (66, 129, 1025, 4097)]


def integer_map(d, seed, n_dead=None):
    """An integer map of d - 1 bins for the exact tests: tests/_large_maps.integer_symmetric with
    some rows dead, plus -- from 63 bins on -- structures that only the mask rules see:
      thin bins   five bins with 2 non-zero cells each (fewer than min_nnz = 5): one shared with
                  the hanger, one with an ordinary bin
      a hanger    its only non-zero cells are the five it shares with the thin bins: it passes
                  min_nnz = 5, and once the thin bins are masked its marginal over the live bins
                  is 0 -- the fixed point of the mask
      far         a bin whose only counts lie 1 and 2 off the diagonal (dead for ignore_diags > 2)
    Row and column d - 1 hold junk (NaN, -1, inf) that nothing may read.
    Returns (matrix, dict of the special bins)."""
    from tests import _large_maps as lm
    rng = numpy.random.default_rng(seed)
    n = d - 1
    dead = None
    if n >= 8:
        k = max(1, n // 16) if n_dead is None else n_dead
        dead = numpy.sort(rng.choice(n, size=k, replace=False))
    m = lm.integer_symmetric(d, rng, dead)
    special = {}
    if n >= 63:
        pool = numpy.setdiff1d(numpy.arange(8, n - 8), dead)
        # eight bins well apart from each other, so that their cells do not collide
        picks = [int(v) for v in pool[numpy.linspace(0, pool.size - 1, 8).astype(int)]]
        thin, hanger, far, anchor = picks[:5], picks[5], picks[6], picks[7]
        for b in thin + [hanger, far]:
            m[b, :] = 0.0
            m[:, b] = 0.0
        for t in thin:
            for other in (hanger, anchor):
                m[t, other] = m[other, t] = 7.0
        for off in (1, 2):
            m[far, far + off] = m[far + off, far] = 11.0
        special = {"thin": thin, "hanger": hanger, "far": far}
    junk = numpy.array([numpy.nan, -1.0, numpy.inf])
    m[n, :] = junk[numpy.arange(d) % 3]
    m[:, n] = junk[(numpy.arange(d) + 1) % 3]
    return m, special
