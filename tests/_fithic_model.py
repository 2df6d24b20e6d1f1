"""The reference of the significance tests (tests/test_fithic_cpu.py, tests/test_gpu_significance.py):
a plain numpy float64 restatement of docs/SPEC.md 2.9 -- bin-level Fit-Hi-C for one chromosome --
and the maps those tests use.  Nothing here touches the library under test.  Results that several
tests need are computed once (`functools.lru_cache`) and must be left unchanged by their users."""
import bisect
import functools
import os

import numpy

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# SPEC 2.9.6: the largest N p the survival function accepts, and the cap of its loop
SF_MAX_MEAN = 1048576.0
SF_MAX_TERMS = 16384
DIST_SCALING = 10000.0

_STIRLERR = numpy.array([
    0.0,
    0.08106146679532725821967026, 0.04134069595540929409382208, 0.02767792568499833914878929,
    0.02079067210376509311152277, 0.01664469118982119216319487, 0.01387612882307074799874573,
    0.01189670994589177009505572, 0.01041126526197209649747857, 0.009255462182712732917728637,
    0.008330563433362871256469319, 0.007573675487951840794972024, 0.006942840107209529865664153,
    0.006408994188004207068439631, 0.005951370112758847735624416, 0.00555473355196280137103869])


# ---- the survival function (SPEC 2.9.6) --------------------------------------------------------
def _stirlerr(n):
    n = numpy.asarray(n, dtype=numpy.float64)
    big = numpy.maximum(n, 16.0)
    nn = big * big
    series = (1.0 / 12.0 - (1.0 / 360.0 - (1.0 / 1260.0 - (1.0 / 1680.0 - (1.0 / 1188.0) / nn) / nn) / nn)
              / nn) / big
    return numpy.where(n <= 15.0, _STIRLERR[numpy.clip(n, 0, 15).astype(numpy.int64)], series)


def _bd0(x, np_):
    with numpy.errstate(all="ignore"):
        v = (x - np_) / (x + np_)
        s = (x - np_) * v
        ej = 2.0 * x * v
        v = v * v
        for j in range(1, 11):
            ej = ej * v
            s = s + ej / (2 * j + 1)
        plain = x * numpy.log(x / np_) + np_ - x
        return numpy.where(numpy.abs(x - np_) < 0.1 * (x + np_), s, plain)


def _pmf(x, n, p, q):
    """P(X = x) for whole 0 < x <= n and 0 < p < 1 (Loader's saddle-point form)."""
    with numpy.errstate(all="ignore"):
        top = numpy.exp(numpy.where(q < 0.1, -_bd0(n, n * p) - n * q, n * numpy.log(p)))
        xs = numpy.where(x == n, 1.0, x)           # (any whole value below n: masked out again)
        ns = numpy.where(x == n, 2.0, n)
        lc = _stirlerr(ns) - _stirlerr(xs) - _stirlerr(ns - xs) - _bd0(xs, ns * p) - _bd0(ns - xs, ns * q)
        lf = numpy.log(2.0 * numpy.pi) + numpy.log(xs) + numpy.log1p(-xs / ns)
        return numpy.where(x == n, top, numpy.exp(lc - 0.5 * lf))


def binomial_sf(k, n, p, return_terms=False):
    """P(X >= k), X ~ Binomial(n, p), elementwise in float64: closed cases, else the pmf at the
    first term and the ratio recurrence (upward from k above the mode; else downward from k - 1
    and 1 - sum) until a term no longer changes the sum.  `return_terms`: also the number of pmf
    values each element summed (0 in a closed case).  Raises if a sum reaches SF_MAX_TERMS."""
    k = numpy.atleast_1d(numpy.asarray(k, dtype=numpy.int64))
    p = numpy.atleast_1d(numpy.asarray(p, dtype=numpy.float64))
    k, p = numpy.broadcast_arrays(k, p)
    n = float(n)
    x = k.astype(numpy.float64)
    out = numpy.full(k.shape, numpy.nan)
    terms = numpy.zeros(k.shape, dtype=numpy.int64)
    valid = (p >= 0.0) & (p <= 1.0)
    out[valid & (p == 1.0)] = 1.0
    out[valid & (p == 0.0)] = 0.0
    out[valid & (x > n)] = 0.0
    out[valid & (k <= 0)] = 1.0
    one = valid & (k == 1) & (x <= n) & (p > 0.0) & (p < 1.0)
    with numpy.errstate(all="ignore"):
        out[one] = -numpy.expm1(n * numpy.log1p(-p[one]))
    todo = numpy.flatnonzero(valid & (k >= 2) & (x <= n) & (p > 0.0) & (p < 1.0))
    if todo.size:
        xs, ps = x[todo], p[todo]
        qs = 1.0 - ps
        up = xs > (n + 1.0) * ps
        r = numpy.where(up, ps / qs, qs / ps)
        j = numpy.where(up, xs, xs - 1.0)
        term = _pmf(j, n, ps, qs)
        total = term.copy()
        count = numpy.ones(todo.size, dtype=numpy.int64)
        live = numpy.ones(todo.size, dtype=bool)
        for _ in range(1, SF_MAX_TERMS):
            with numpy.errstate(all="ignore"):
                term = term * numpy.where(up, (n - j) / (j + 1.0) * r, j / (n - j + 1.0) * r)
            j = j + numpy.where(up, 1.0, -1.0)
            s1 = total + term
            live &= s1 != total
            if not live.any():
                break
            total = numpy.where(live, s1, total)
            count += live
        else:
            raise RuntimeError("binomial_sf: a tail sum reached SF_MAX_TERMS")
        out[todo] = numpy.where(up, total, 1.0 - total)
        terms[todo] = count
    return (out, terms) if return_terms else out


@functools.lru_cache(maxsize=None)
def truth_table():
    """tests/golden/binomial_sf_truth.npz (tools/make_binomial_sf_truth.py): k (int64), n, p and the
    80-digit tail sum rounded to float64, row by row; every row has its own n."""
    z = numpy.load(os.path.join(GOLDEN, "binomial_sf_truth.npz"))
    out = {name: z[name] for name in ("k", "n", "p", "truth")}
    for a in out.values():
        a.flags.writeable = False
    return out


# the model's worst relative error over the truth table, measured (test_fithic_cpu prints it):
# 1.64e-13 (row 354: k = 1,007,960, n = 1e8, p = 0.01) -- see docs/MEASUREMENTS.md; the asserted
# bounds are multiples of THIS figure
MODEL_WORST = 1.64e-13
TINY_TRUTH, TINY_RESULT = 1e-290, 1e-289


def table_errors(got):
    """(worst relative error over the rows whose truth is >= TINY_TRUTH, its row, whether every
    row below it has a result <= TINY_RESULT, the share of such rows)."""
    t = truth_table()
    truth = t["truth"]
    big = truth >= TINY_TRUTH
    with numpy.errstate(all="ignore"):
        rel = numpy.where(truth[big] == 0, numpy.abs(got[big]), numpy.abs(got[big] / truth[big] - 1.0))
    rel = numpy.where(numpy.isnan(rel), numpy.inf, rel)
    worst = int(numpy.argmax(rel)) if rel.size else -1
    tiny_ok = bool(numpy.all((got[~big] <= TINY_RESULT) & (got[~big] >= 0.0)))
    return (float(rel[worst]) if rel.size else 0.0, int(numpy.flatnonzero(big)[worst]) if rel.size else -1,
            tiny_ok, float((~big).mean()))


# ---- the host steps (SPEC 2.9.1 - 2.9.4) -------------------------------------------------------
def in_range(n, resolution, min_dist, max_dist):
    """The diagonals k of an n-bin map with min_dist < k r <= max_dist."""
    return [k for k in range(n) if min_dist < k * resolution <= max_dist]


def tallies(m, n, ks):
    """(P, O) for k = 0 .. n - 1: possible pairs n - k; observed counts of diagonal k of the leading
    n x n block, 0 outside the range."""
    possible = numpy.array([n - k for k in range(n)], dtype=numpy.float64)
    observed = numpy.zeros(n)
    for k in ks:
        observed[k] = numpy.trace(m[:n, :n], k)
    return possible, observed


def offending_cells(m, n, ks):
    """The number of counted cells that are not raw counts."""
    bad = 0
    for k in ks:
        d = numpy.diagonal(m[:n, :n], k)
        with numpy.errstate(invalid="ignore"):
            bad += int((~(numpy.isfinite(d) & (d >= 0) & (d == numpy.floor(d)))).sum())
    return bad


def equal_occupancy(possible, observed, ks, resolution, n_bins):
    """SPEC 2.9.2: the in-range diagonals, ascending, are dealt into bins of about N / n_bins
    reads each.  Returns (x, y): the bins' pair-weighted mean distance and mean contact
    probability per pair."""
    total = float(sum(observed[k] for k in ks))
    desired = float(int(total) // int(n_bins))
    xs, ys, pending = [], [], []
    seen = acc = 0.0
    closed = 0
    for k in ks:
        seen += observed[k]
        pending.append(k)
        if observed[k] >= desired or acc + observed[k] >= desired:
            closed += 1
            if closed < n_bins:
                desired = 1.0 * (total - seen) / (n_bins - closed)
            pairs = reads = dist = 0.0
            for b in pending:
                pairs += possible[b]
                reads += observed[b]
                dist += 1.0 * possible[b] * (b * resolution / DIST_SCALING)
            ys.append((reads / pairs) / total)
            xs.append(DIST_SCALING * (dist / pairs))
            pending, acc = [], 0.0
        else:
            acc += observed[k]
    return numpy.array(xs), numpy.array(ys)


def pava_nonincreasing(y):
    """The least-squares non-increasing fit of y (unit weights), by pooling adjacent violators."""
    blocks = []                                   # [sum, length]
    for v in numpy.asarray(y, dtype=numpy.float64):
        blocks.append([float(v), 1])
        while len(blocks) > 1 and blocks[-2][0] / blocks[-2][1] < blocks[-1][0] / blocks[-1][1]:
            s, c = blocks.pop()
            blocks[-1][0] += s
            blocks[-1][1] += c
    return numpy.concatenate([numpy.full(c, s / c) for s, c in blocks]) if blocks else numpy.zeros(0)


def spline_table(x, y, n, resolution, ks):
    """SPEC 2.9.3 - 2.9.4: (spline_x, spline_y, f): the smoothing spline at the in-range distances
    inside [min x, max x], made non-increasing, and the lookup table f_k, k = 0 .. n - 1."""
    from scipy.interpolate import UnivariateSpline
    spline = UnivariateSpline(x, y, s=min(y) ** 2)
    lo, hi = min(x), max(x)
    sx = [k * resolution for k in ks if lo <= k * resolution <= hi]
    sy = pava_nonincreasing(spline(sx))
    f = numpy.empty(n)
    for k in range(n):
        d = min(max(k * resolution, lo), hi)
        f[k] = sy[min(bisect.bisect_left(sx, d), len(sx) - 1)]
    return numpy.array(sx, dtype=numpy.float64), sy, f


def bh(p_sorted, n_tests):
    """q[i] = max(q[i - 1], min(p[i] n / (i + 1), 1)) (docs/SPEC.md: benjamini_hochberg)."""
    q = numpy.minimum(p_sorted * float(n_tests) / numpy.arange(1, p_sorted.shape[0] + 1), 1.0)
    return numpy.maximum.accumulate(q)


def fithic(m, bias, resolution, min_dist=0, max_dist=10000000, n_bins=100, bias_range=(0.5, 2.0),
           prior=None):
    """SPEC 2.9 end to end on the (n + 1)^2 matrix `m`.  `prior`: a table f_k to use in place of
    the spline's (the device tests hand the library's own to both sides, so that the lists are
    compared under one prior).  Returns a dict."""
    m = numpy.asarray(m, dtype=numpy.float64)
    n = m.shape[0] - 1
    bias = numpy.ones(n) if bias is None else numpy.asarray(bias, dtype=numpy.float64)
    ks = in_range(n, resolution, min_dist, max_dist)
    if not ks:
        raise ValueError("empty range")
    if offending_cells(m, n, ks):
        raise ValueError("significance needs raw counts")
    possible, observed = tallies(m, n, ks)
    n_reads = float(sum(observed[k] for k in ks))
    n_tests = int(sum(possible[k] for k in ks))
    out = {"n_reads": n_reads, "n_tests": n_tests, "ks": ks}
    if prior is None:
        x, y = equal_occupancy(possible, observed, ks, resolution, n_bins)
        if len(x) < 4:
            raise ValueError("fewer than 4 binning points")
        sx, sy, prior = spline_table(x, y, n, resolution, ks)
        out.update(bins_x=x, bins_y=y, spline_x=sx, spline_y=sy)
    prior = numpy.asarray(prior, dtype=numpy.float64)
    out["prior"] = prior
    lo, hi = (-numpy.inf, numpy.inf) if bias_range is None else bias_range
    # the cells of the upper triangle in range, row-major (numpy.nonzero's order)
    i, j = numpy.nonzero(numpy.triu(numpy.ones((n, n), dtype=bool), ks[0])
                         & ~numpy.triu(numpy.ones((n, n), dtype=bool), ks[-1] + 1))
    c = m[i, j]
    with numpy.errstate(invalid="ignore"):
        pi = prior[j - i] * bias[i] * bias[j]
        listed = ((c >= 1) & (bias[i] >= lo) & (bias[i] <= hi) & (bias[j] >= lo) & (bias[j] <= hi)
                  & (pi >= 0.0) & (pi <= 1.0))
    rows, cols, counts, pis = i[listed], j[listed], c[listed], pi[listed]
    if pis.size and (n_reads * pis[pis < 1.0]).max(initial=0.0) > SF_MAX_MEAN:
        raise ValueError("N * prior above the limit")
    p = binomial_sf(counts.astype(numpy.int64), n_reads, pis) if pis.size else numpy.zeros(0)
    order = numpy.argsort(p, kind="stable")
    q = numpy.empty_like(p)
    q[order] = bh(p[order], n_tests)
    out.update(rows=rows, cols=cols, counts=counts, p=p, q=q)
    return out


# ---- the maps ----------------------------------------------------------------------------------
def random_map(n, seed, mean=6.0, zero_share=0.3):
    """An (n + 1)^2 symmetric map of whole counts that decay with distance, a share of the cells
    0; row and column n hold NaN, -1 and inf by turns (never read)."""
    rng = numpy.random.default_rng(seed)
    i = numpy.arange(n)
    k = numpy.abs(i[:, None] - i[None, :])
    m = rng.poisson(mean * 8.0 / (k + 1.0) + 0.6).astype(numpy.float64)
    m[rng.random((n, n)) < zero_share] = 0.0
    m = numpy.triu(m)
    m = m + numpy.triu(m, 1).T
    full = numpy.zeros((n + 1, n + 1))
    full[:n, :n] = m
    junk = numpy.array([numpy.nan, -1.0, numpy.inf])
    full[n, :] = junk[numpy.arange(n + 1) % 3]
    full[:, n] = junk[(numpy.arange(n + 1) + 1) % 3]
    return full


def random_bias(n, seed):
    """A bias vector in [0.7, 1.4] with (n >= 4) one dead bin (NaN) and one bin outside [0.5, 2]."""
    rng = numpy.random.default_rng(seed + 1000)
    b = rng.uniform(0.7, 1.4, n)
    if n >= 4:
        b[n // 3] = numpy.nan
        b[(2 * n) // 3] = 2.5
    return b


def decay_prior(n, n_reads, zero_at=None, above_one_at=None, nan_at=None):
    """A hand-made prior table: ~ 1 / (k + 1), scaled so that N f_0 is a few counts; f = 0 at
    `zero_at`, 4 (a prior above 1 whatever the biases in [0.5, 2]) at `above_one_at`, NaN at
    `nan_at`, each where the table is that long."""
    f = 8.0 / (numpy.arange(n) + 1.0) / max(n_reads, 1.0)
    for at, value in ((zero_at, 0.0), (above_one_at, 4.0), (nan_at, numpy.nan)):
        if at is not None and at < n:
            f[at] = value
    return f


def long_rows_map(n=2100, seed=7):
    """An (n + 1)^2 map of whole counts whose rows hold few stored cells (a band of 12 diagonals,
    a third of it empty) except four: rows 5, 400 and 800 hold exactly 1,023, 1,024 and 1,025
    non-zero cells of the symmetric leading block -- the last size that fits one 1,024-entry
    segment of the triples index, and the first two past it -- and row 50 holds all n of them
    (three segments).  Row and column n hold junk as in random_map.  READ-ONLY (shared)."""
    rng = numpy.random.default_rng(seed)
    i = numpy.arange(n)
    k = numpy.abs(i[:, None] - i[None, :])
    upper = numpy.triu(rng.poisson(30.0 / (k + 1.0) + 0.5) * ((k <= 12) & (rng.random((n, n)) > 0.33)))
    m = (upper + numpy.triu(upper, 1).T).astype(numpy.float64)
    m[50, :] = m[:, 50] = 1.0 + rng.integers(0, 5, n)
    special = {5: 1023, 400: 1024, 800: 1025}
    for row, want in special.items():
        free = numpy.flatnonzero((m[row] == 0) & ~numpy.isin(i, list(special)))
        add = rng.choice(free, size=want - int((m[row] != 0).sum()), replace=False)
        m[row, add] = m[add, row] = 1.0 + rng.integers(0, 5, add.shape[0])
    full = numpy.zeros((n + 1, n + 1))
    full[:n, :n] = m
    junk = numpy.array([numpy.nan, -1.0, numpy.inf])
    full[n, :] = junk[numpy.arange(n + 1) % 3]
    full[:, n] = junk[(numpy.arange(n + 1) + 1) % 3]
    full.flags.writeable = False
    return full


def triples_of(m, resolution, seed, duplicates=True):
    """The upper triangle of the (n + 1)^2 map `m`'s leading block as shuffled Rao triples
    [pos_i, pos_j, count], either orientation; with `duplicates` some pairs come twice (the LAST
    holds the map's value) and one pair touches bin n."""
    rng = numpy.random.default_rng(seed + 2000)
    n = m.shape[0] - 1
    i, j = numpy.nonzero(numpy.triu(m[:n, :n]))
    v = m[i, j]
    flip = rng.random(i.shape[0]) < 0.5
    a, b = numpy.where(flip, j, i), numpy.where(flip, i, j)
    order = rng.permutation(i.shape[0])
    t = numpy.column_stack([a[order] * float(resolution), b[order] * float(resolution), v[order]])
    if duplicates and t.shape[0]:
        pick = rng.choice(t.shape[0], size=max(1, t.shape[0] // 7), replace=False)
        early = t[pick].copy()
        early[:, 2] += 3.0                       # an earlier, different value: must lose
        early[:, :2] = early[:, 1::-1]           # and in the other orientation
        t = numpy.concatenate([early, t, [[n * float(resolution), 0.0, 7.0]]])
    return numpy.ascontiguousarray(t)


PLANTED_N, PLANTED_RES, PLANTED_SEED = 400, 10000, 0
PLANTED_TOTAL, PLANTED_CELLS, PLANTED_BOOST = 3e6, 24, 10.0


@functools.lru_cache(maxsize=None)
def planted_map():
    """The end-to-end map of the issue: n = 400, r = 10,000; counts Poisson with mean
    proportional to b_i b_j / (k + 1), b uniform in [0.7, 1.4], 3e6 reads in the upper triangle;
    24 planted cells at k >= 5 whose unboosted mean lies in (0.5, 20), boosted x 10.
    Returns ((n + 1)^2 map, bias, planted (24, 2) bins)."""
    n = PLANTED_N
    rng = numpy.random.default_rng(PLANTED_SEED)
    b = rng.uniform(0.7, 1.4, n)
    i = numpy.arange(n)
    k = i[None, :] - i[:, None]
    mean = numpy.triu(b[:, None] * b[None, :] / (numpy.abs(k) + 1.0))
    mean *= PLANTED_TOTAL / mean.sum()
    cand = numpy.argwhere((k >= 5) & (mean > 0.5) & (mean < 20.0))
    planted = cand[rng.choice(cand.shape[0], size=PLANTED_CELLS, replace=False)]
    mean[planted[:, 0], planted[:, 1]] *= PLANTED_BOOST
    upper = rng.poisson(mean).astype(numpy.float64)
    full = numpy.zeros((n + 1, n + 1))
    full[:n, :n] = upper + numpy.triu(upper, 1).T
    for a in (full, b, planted):
        a.flags.writeable = False
    return full, b, planted


@functools.lru_cache(maxsize=None)
def planted_model():
    m, b, _ = planted_map()
    return fithic(m, b, PLANTED_RES)
