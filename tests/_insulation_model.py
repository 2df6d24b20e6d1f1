"""Test-only: docs/SPEC.md 2.13 restated in numpy -- the insulation sums and counts of a map, the
closed form of an unclipped diamond's cells, the test maps and the planted-domain map.  Never
imported by the package.

The order of summation is part of the definition: per row a of bin i's diamond, top to bottom, a
row partial of M_ab (x_a x_b) over the row's live cells, left to right; then the partials top to
bottom; every accumulator from +0.0.  `sums_counts` does that through numpy.cumsum, which adds
strictly in sequence (as tests/_coarsen_model.py relies on), over the masked, weighted block of
every bin: along its columns, then down its last column.  A masked cell is a 0.0, and adding a 0.0
to an accumulator that started at +0.0 never changes its bits.  `sums_counts_loops` is the same
definition as three plain loops that skip what is not live, for small n."""
import numpy


def weights(n, bias=None):
    """x = 1 / bias, 0 where the bias is NaN; all ones without a bias."""
    if bias is None:
        return numpy.ones(n)
    b = numpy.asarray(bias, dtype=numpy.float64)[:n]
    x = numpy.zeros(n)
    ok = ~numpy.isnan(b)
    with numpy.errstate(divide="ignore"):
        x[ok] = 1.0 / b[ok]
    return x


def weighted_cells(M, n, g, x):
    """(n, n): M_ab (x_a x_b) at the live cells a <= b - g of the leading block, 0.0 elsewhere (a
    dead cell is selected out, whatever it holds)."""
    a, b = numpy.indices((n, n))
    live = (b - a >= g) & (x[:, None] != 0.0) & (x[None, :] != 0.0)
    W = numpy.zeros((n, n))
    with numpy.errstate(invalid="ignore", over="ignore"):
        W[live] = (numpy.asarray(M, dtype=numpy.float64)[:n, :n] * (x[:, None] * x[None, :]))[live]
    return W


def counts_of(n, w, g, x):
    """cnt_i from the prefix count L of the live bins: for each live row a of the diamond, the live
    bins of [max(i, a + g), hi_i]."""
    L = numpy.concatenate([[0], numpy.cumsum(x != 0.0)]).astype(numpy.int64)
    out = numpy.zeros(n, dtype=numpy.int64)
    for i in range(n):
        hi = min(n - 1, i + w - 1)
        a = numpy.arange(max(0, i - w + 1), i + 1)
        first = numpy.maximum(i, a + g)
        ok = (x[a] != 0.0) & (first <= hi)
        out[i] = (L[hi + 1] - L[numpy.minimum(first, hi + 1)])[ok].sum()
    return out


def sums_counts(M, n, w, g, bias=None):
    """(sums float64, counts int64) of SPEC 2.13 over bins 0 .. n - 1 of the (n + 1)^2 matrix M."""
    n, w, g = int(n), int(w), int(g)
    x = weights(n, bias)
    W = weighted_cells(M, n, g, x)
    sums = numpy.zeros(n)
    with numpy.errstate(invalid="ignore", over="ignore"):
        for i in range(n):
            lo, hi = max(0, i - w + 1), min(n - 1, i + w - 1)
            top = min(i, hi - g)                      # (the rows below have no cell: +0.0 each)
            if top < lo:
                continue
            block = W[lo:top + 1, i:hi + 1]
            cells = numpy.concatenate([numpy.zeros((block.shape[0], 1)), block], axis=1)
            rows = numpy.concatenate([[0.0], numpy.cumsum(cells, axis=1)[:, -1]])
            sums[i] = numpy.cumsum(rows)[-1]
    return sums, counts_of(n, w, g, x)


def sums_counts_loops(M, n, w, g, bias=None):
    """The definition as three loops, skipping every cell that is not live."""
    n, w, g = int(n), int(w), int(g)
    M = numpy.asarray(M, dtype=numpy.float64)
    x = weights(n, bias)
    sums, counts = numpy.zeros(n), numpy.zeros(n, dtype=numpy.int64)
    with numpy.errstate(invalid="ignore", over="ignore"):
        for i in range(n):
            total = numpy.float64(0.0)
            for a in range(max(0, i - w + 1), i + 1):
                if x[a] == 0.0:
                    continue
                r = numpy.float64(0.0)
                for b in range(max(i, a + g), min(n - 1, i + w - 1) + 1):
                    if x[b] == 0.0:
                        continue
                    r = r + M[a, b] * (x[a] * x[b])
                    counts[i] += 1
                total = total + r
            sums[i] = total
    return sums, counts


def full_cells_enumerated(w, g):
    """The cells (a, b) of an unclipped diamond, 0 <= a < w <= b + 1 < 2 w, with b - a >= g."""
    return sum(1 for a in range(w) for b in range(w - 1, 2 * w - 1) if b - a >= g)


def poisoned_bins(n, w, g, r, c):
    """The bins whose diamond holds the upper cell (r, c), r <= c."""
    if c - r < g:
        return numpy.zeros(0, dtype=numpy.int64)
    return numpy.arange(max(r, c - w + 1), min(c, r + w - 1) + 1, dtype=numpy.int64)


# ---- the test maps -------------------------------------------------------------------------------
def integer_map(n_bins, seed):
    """A symmetric (n_bins + 1)^2 map of small integer counts, a third of them 0, with a junk row
    and column n_bins that no call may read.  Every order of summation gives the same bits."""
    r = numpy.random.default_rng(seed)
    d = n_bins + 1
    U = numpy.triu(r.integers(0, 50, (d, d)) * (r.random((d, d)) < 0.67)).astype(numpy.float64)
    M = U + numpy.triu(U, 1).T
    M[n_bins, :] = M[:, n_bins] = 7.0
    return M


def wide_map(n_bins, seed):
    """The same shape with random mantissas times 10^e, e an integer in [-6, 6], a quarter of the
    cells 0: the sum of a diamond depends on the order of its adds."""
    r = numpy.random.default_rng(seed)
    d = n_bins + 1
    vals = r.uniform(1.0, 10.0, (d, d)) * 10.0 ** r.integers(-6, 7, (d, d))
    U = numpy.triu(vals * (r.random((d, d)) < 0.75))
    M = U + numpy.triu(U, 1).T
    M[n_bins, :] = M[:, n_bins] = 3.5
    return M


def nan_bias(n, seed, share=0.1):
    """A bias of exp(N(0, 0.3)) with a share of NaN bins (at least one where n allows)."""
    r = numpy.random.default_rng(seed)
    b = numpy.exp(r.normal(0.0, 0.3, n))
    dead = r.random(n) < share
    if n > 2:
        dead[r.integers(0, n)] = True
    b[dead] = numpy.nan
    return b


def triples_of(M, n_bins, resolution, keep_zeros=0.0, seed=0):
    """The upper triangle of M's leading block as triples [i R, j R, v]: every non-zero cell, and
    a share `keep_zeros` of the zero cells as stored zeros."""
    r = numpy.random.default_rng(seed)
    U = numpy.asarray(M)[:n_bins, :n_bins]
    take = numpy.triu(numpy.ones(U.shape, dtype=bool)) & ((U != 0) | (r.random(U.shape) < keep_zeros))
    i, j = numpy.nonzero(take)
    return numpy.stack([i * float(resolution), j * float(resolution), U[i, j]], axis=1).reshape(-1, 3)


# ---- planted domains -----------------------------------------------------------------------------
def planted_map(n, w, seed):
    """(M, bias, borders): Poisson counts of 200 (1 + |i - j|)^-1.08 bias_i bias_j, the rate
    multiplied by 0.35 for a pair on two sides of a domain border; bias = exp(N(0, 0.3)); domain
    lengths uniform in [3 w, 6 w); a border nearer than 2 w to either end is dropped (not planted:
    its two domains are one).  A border at
    bin p separates bins < p from bins >= p.  M is (n + 1)^2 with a zero padding."""
    r = numpy.random.default_rng(seed)
    bias = numpy.exp(r.normal(0.0, 0.3, n))
    cuts, p = [], 0
    while True:
        p += int(r.integers(3 * w, 6 * w))
        if p >= n:
            break
        cuts.append(p)
    borders = numpy.asarray([c for c in cuts if 2 * w <= c <= n - 2 * w], dtype=numpy.int64)
    domain = numpy.searchsorted(borders, numpy.arange(n), side="right")
    i, j = numpy.indices((n, n))
    rate = 200.0 * (1.0 + numpy.abs(i - j)) ** -1.08 * numpy.outer(bias, bias)
    rate = numpy.where(domain[:, None] != domain[None, :], 0.35 * rate, rate)
    U = numpy.triu(r.poisson(rate)).astype(numpy.float64)
    M = numpy.zeros((n + 1, n + 1))
    M[:n, :n] = U + numpy.triu(U, 1).T
    return M, bias, borders


PLANTED = [(400, 10, 1), (600, 20, 2), (1000, 25, 3)]          # (n, w, seed)


def planted_condition(bins, strengths, borders, threshold=0.5):
    """(every planted border has a boundary of strength >= threshold within +-1 bin, no other
    boundary reaches the threshold; the weakest planted strength, the strongest other)."""
    bins, strengths = numpy.asarray(bins), numpy.asarray(strengths)
    near = numpy.zeros(bins.shape[0], dtype=bool)
    weakest = numpy.inf
    for p in borders:
        # a border between bins p - 1 and p: the minimum sits on one of them
        hit = (bins >= p - 1) & (bins <= p + 1)
        near |= hit
        weakest = min(weakest, strengths[hit].max() if hit.any() else -numpy.inf)
    other = strengths[~near].max() if (~near).any() else 0.0
    return bool(weakest >= threshold and other < threshold), float(weakest), float(other)
