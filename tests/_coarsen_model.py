"""Test-only: docs/SPEC.md 2.12 restated in numpy -- the pooled map (dense and pixel list), the
cell counts of how='mean', and the two structure helpers.  Never imported by the package.

The order of summation is part of the definition: per fine row a of a block, top to bottom, a row
partial of its cells left to right; then the partials top to bottom; every accumulator from +0.0.
`pooled` does that as k^2 vectorised adds over P[a::k, b::k] of the zero-padded upper triangle
(adding a 0.0 to an accumulator that started at +0.0 never changes its bits, so the zero cells
below the diagonal and beyond n_bins are the same as leaving them out); `pooled_by_cumsum` does
the same adds through numpy.cumsum (strictly left to right) for the factors where k^2 numpy calls
would take seconds."""
import numpy

K2_ADDS_UP_TO = 40           # `pooled` takes the k^2-adds form up to this factor


def n_coarse(n_bins, k):
    return -(-int(n_bins) // int(k))


def _padded_upper(M, n_bins, k):
    """The upper triangle (diagonal included) of the leading n_bins x n_bins block, zero-padded to
    nc k rows and columns."""
    n, nc = int(n_bins), n_coarse(n_bins, k)
    P = numpy.zeros((nc * k, nc * k))
    P[:n, :n] = numpy.triu(numpy.asarray(M, dtype=numpy.float64)[:n, :n])
    return P


def _mirror(U, nc):
    """(nc + 1)^2: the upper triangle U, its mirror below, a zero padding row and column."""
    out = numpy.zeros((nc + 1, nc + 1))
    iu = numpy.triu_indices(nc)
    out[:nc, :nc][iu] = U[iu]
    out[:nc, :nc].T[iu] = U[iu]
    return out


def pooled_sums_k2(M, n_bins, k):
    """(nc, nc): the pooled sums of the upper triangle by k^2 vectorised adds (lower: junk 0)."""
    nc = n_coarse(n_bins, k)
    P = _padded_upper(M, n_bins, k)
    total = numpy.zeros((nc, nc))
    with numpy.errstate(invalid="ignore", over="ignore"):
        for a in range(k):                       # fine rows, top to bottom
            r = numpy.zeros((nc, nc))
            for b in range(k):                   # the row's cells, left to right
                r += P[a::k, b::k]
            total += r
    return total


def pooled_sums_cumsum(M, n_bins, k):
    """The same adds in the same order through numpy.cumsum, which adds strictly in sequence; a
    leading +0.0 makes the first add the accumulator's start."""
    nc = n_coarse(n_bins, k)
    P = _padded_upper(M, n_bins, k).reshape(nc, k, nc, k)          # [I, a, J, b]
    with numpy.errstate(invalid="ignore", over="ignore"):
        cells = numpy.concatenate([numpy.zeros((nc, k, nc, 1)), P], axis=3)
        r = numpy.cumsum(cells, axis=3)[:, :, :, -1]               # [I, a, J]
        rows = numpy.concatenate([numpy.zeros((nc, 1, nc)), r], axis=1)
        return numpy.cumsum(rows, axis=1)[:, -1, :]


def cell_counts(n_bins, k):
    """(nc, nc) float64: the fine cells pooled into (I, J), I <= J: |I| |J| off the diagonal,
    |I| (|I| + 1) / 2 on it (1 below the diagonal, which nobody reads)."""
    n, nc = int(n_bins), n_coarse(n_bins, k)
    size = numpy.minimum(k, n - numpy.arange(nc, dtype=numpy.int64) * k)
    c = numpy.triu(numpy.outer(size, size), 1) + numpy.diag(size * (size + 1) // 2)
    c[numpy.tril_indices(nc, -1)] = 1
    return c.astype(numpy.float64)


def pooled(M, n_bins, k, how="sum"):
    """The (nc + 1)^2 pooled matrix of the (n_bins + 1)^2 matrix M (SPEC 2.12)."""
    k = int(k)
    nc = n_coarse(n_bins, k)
    if nc == 0:
        return numpy.zeros((1, 1))
    k_eff = min(k, max(int(n_bins), 1))          # (beyond n_bins: one bin, as n_bins itself)
    sums = (pooled_sums_k2 if k_eff <= K2_ADDS_UP_TO else pooled_sums_cumsum)(M, n_bins, k_eff)
    if how == "mean":
        with numpy.errstate(invalid="ignore", over="ignore"):
            sums = sums / cell_counts(n_bins, k_eff)
    else:
        assert how == "sum"
    return _mirror(sums, nc)


def reshape_sum(M, n_bins, k):
    """What a numpy user would write: reshape(nc, k, nc, k).sum((1, 3)) of the symmetric block with
    the diagonal blocks corrected to count every fine pair once.  Equal to `pooled` on integer
    maps; another order of summation otherwise."""
    n, nc = int(n_bins), n_coarse(n_bins, k)
    S = numpy.zeros((nc * k, nc * k))
    U = numpy.triu(numpy.asarray(M, dtype=numpy.float64)[:n, :n])
    S[:n, :n] = U + numpy.triu(U, 1).T
    full = S.reshape(nc, k, nc, k).sum(axis=(1, 3))
    D = numpy.zeros((nc * k, nc * k))
    D[:n, :n] = numpy.diag(numpy.diag(U))
    diag = D.reshape(nc, k, nc, k).sum(axis=(1, 3))
    full[numpy.diag_indices(nc)] = (numpy.diag(full) + numpy.diag(diag)) / 2.0
    return _mirror(full, nc)


# ---- the pixel-list form -------------------------------------------------------------------------
def stored_cells(triples, resolution, n_bins):
    """(i, j, v) of the canonical index: bins of the nan_to_num'ed positions, the unordered pair,
    both bins below n_bins, the LAST triple of a pair; sorted by (i, j), i <= j."""
    t = numpy.nan_to_num(numpy.asarray(triples, dtype=numpy.float64).reshape(-1, 3))
    a = (t[:, 0] / resolution).astype(numpy.int64)
    b = (t[:, 1] / resolution).astype(numpy.int64)
    i, j = numpy.minimum(a, b), numpy.maximum(a, b)
    keep = j < n_bins
    i, j, v = i[keep], j[keep], t[keep, 2]
    key = i * max(int(n_bins), 1) + j
    _, first_rev = numpy.unique(key[::-1], return_index=True)
    last = key.shape[0] - 1 - first_rev
    return i[last], j[last], v[last]


def pooled_triples(triples, resolution, n_bins, k, how="sum"):
    """(pooled triples, nc) of SPEC 2.12: one [I R, J R, value] per pooled upper cell with at
    least one stored fine cell, I ascending, then J; the values are `pooled`'s of the matrix the
    triples define."""
    k = int(k)
    nc = n_coarse(n_bins, k)
    i, j, v = stored_cells(triples, resolution, n_bins)
    M = numpy.zeros((int(n_bins) + 1, int(n_bins) + 1))
    M[i, j] = v
    P = pooled(M, n_bins, k, how)
    cells = numpy.unique((i // k) * max(nc, 1) + (j // k))
    I, J = cells // max(nc, 1), cells % max(nc, 1)
    R = float(resolution * k)
    return numpy.stack([I * R, J * R, P[I, J]], axis=1).reshape(-1, 3), nc


# ---- the test maps -------------------------------------------------------------------------------
def integer_map(n_bins, seed):
    """A symmetric (n_bins + 1)^2 map of small integer counts, a third of them 0, with a junk
    (non-zero) row and column n_bins that no call may read.  Every order of summation gives the
    same bits."""
    r = numpy.random.default_rng(seed)
    d = n_bins + 1
    U = numpy.triu(r.integers(0, 50, (d, d)) * (r.random((d, d)) < 0.67)).astype(numpy.float64)
    M = U + numpy.triu(U, 1).T
    M[n_bins, :] = M[:, n_bins] = 7.0
    return M


def wide_map(n_bins, seed):
    """The same shape with values uniform(0.5, 1) 2^e, e an integer in [-20, 20], a quarter of the
    cells 0: the sum of a block depends on the order of its adds."""
    r = numpy.random.default_rng(seed)
    d = n_bins + 1
    vals = r.uniform(0.5, 1.0, (d, d)) * 2.0 ** r.integers(-20, 21, (d, d))
    U = numpy.triu(vals * (r.random((d, d)) < 0.75))
    M = U + numpy.triu(U, 1).T
    M[n_bins, :] = M[:, n_bins] = 3.5
    return M


def wide_seed(n_bins, k):
    return 7 * n_bins + k


# (n_bins, factor) at which tests/test_coarsen_cpu.py shows that the order of summation changes the
# bits of wide_map(n_bins, wide_seed(n_bins, factor)); tests/test_gpu_coarsen.py runs them all
ORDER_CASES = [(63, 2), (63, 7), (64, 16), (65, 64), (129, 10), (257, 5), (257, 257), (1000, 100),
               (1025, 3), (1025, 64), (1025, 1026)]


def triples_of(M, n_bins, resolution, keep_zeros=0.0, seed=0):
    """The upper triangle of M's leading block as triples [i R, j R, v]: every non-zero cell, and
    a share `keep_zeros` of the zero cells as stored zeros."""
    r = numpy.random.default_rng(seed)
    U = numpy.asarray(M)[:n_bins, :n_bins]
    take = numpy.triu(numpy.ones(U.shape, dtype=bool)) & ((U != 0) | (r.random(U.shape) < keep_zeros))
    i, j = numpy.nonzero(take)
    return numpy.stack([i * float(resolution), j * float(resolution), U[i, j]], axis=1).reshape(-1, 3)


# ---- the structure helpers -----------------------------------------------------------------------
def coarsen_structure(X, k):
    """Per coarse bin the mean of its rows, added top to bottom; rows with a non-finite
    coordinate left out, NaN where none is left.  Plain loops."""
    X = numpy.asarray(X, dtype=numpy.float64)
    n = X.shape[0]
    out = numpy.full((n_coarse(n, k), 3), numpy.nan)
    for I in range(out.shape[0]):
        s, m = numpy.zeros(3), 0
        for a in range(I * k, min((I + 1) * k, n)):
            if numpy.isfinite(X[a]).all():
                s, m = s + X[a], m + 1
        if m:
            out[I] = s / m
    return out


def prolong_structure(Xc, k, n_bins):
    """numpy.interp of every coordinate at the fine bins over the centres (lo + hi - 1) / 2 of the
    coarse bins whose row is finite."""
    Xc = numpy.asarray(Xc, dtype=numpy.float64)
    centre = numpy.array([(I * k + min((I + 1) * k, n_bins) - 1) / 2.0 for I in range(Xc.shape[0])])
    ok = numpy.isfinite(Xc).all(axis=1)
    out = numpy.full((n_bins, 3), numpy.nan)
    if ok.any():
        for c in range(3):
            out[:, c] = numpy.interp(numpy.arange(n_bins), centre[ok], Xc[ok, c])
    return out
