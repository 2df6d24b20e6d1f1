"""The wish-distance matrix every input route of the solver has to leave in its units, written
from the rules of docs/SPEC.md 2.1 and include/blueberry_hip.h in numpy float64, the inputs the
route tests run on, and the list of cases tests/test_gpu_input_routes.py and
tests/test_input_model_cpu.py share.  No library code: nothing here imports blueberry_amd.

The rules:
  value      finite and positive, else no constraint (0); kind='counts': v ** (-1 / alpha); a
             distance below the wish floor (1e-30 fp32, 1e-290 fp64) or above the largest finite
             value of the run's dtype is no constraint; then the rounding to the dtype
  dense      only the upper triangle is read
  entries    a diagonal entry is skipped; of several entries of one unordered pair, in either
             orientation, the LAST one counts (an explicit 0 included)
  triples    numpy.nan_to_num of every value read; bin = C truncation of pos / resolution
  KR         v / (kr[i] * kr[j] * ke[j - i]) in that operation order for i < j, then nan_to_num
  coords     delta_ij = |x*_i - x*_j|, then the flush of the value rule
"""
import functools

import numpy

from tests import _spectral_model as sm

DBL_MAX = float(numpy.finfo(numpy.float64).max)
FLT_MAX = float(numpy.finfo(numpy.float32).max)
WISH_FLOOR = {"float32": 1e-30, "float64": 1e-290}          # SPEC 2.1
WISH_CEILING = {"float32": FLT_MAX, "float64": DBL_MAX}     # SPEC 2.1
POW2 = numpy.array([0.0, 0.25, 0.5, 1.0, 2.0])
RESOLUTION = 5000


# ---- the rules --------------------------------------------------------------------------------
def nan_to_num(a):
    """numpy.nan_to_num written out: NaN -> 0, +-inf -> the largest double of that sign."""
    out = numpy.array(a, dtype=numpy.float64)
    out[out != out] = 0.0
    out[out == numpy.inf] = DBL_MAX
    out[out == -numpy.inf] = -DBL_MAX
    return out


def flush_wish(d, dtype):
    """A distance as the units hold it, widened to float64 again."""
    d = numpy.asarray(d, dtype=numpy.float64)
    keep = (d >= WISH_FLOOR[dtype]) & (d <= WISH_CEILING[dtype])
    return numpy.where(keep, d, 0.0).astype(dtype).astype(numpy.float64)


def wish_from_value(v, kind, alpha, dtype):
    v = numpy.asarray(v, dtype=numpy.float64)
    ok = numpy.isfinite(v) & (v > 0.0)
    d = numpy.zeros_like(v)
    d[ok] = v[ok] ** (-1.0 / alpha) if kind == "counts" else v[ok]
    return flush_wish(d, dtype)


def bins_of(pos, resolution):
    """(int)(nan_to_num(pos) / resolution); ValueError where an int cannot hold the quotient."""
    q = nan_to_num(pos) / float(resolution)
    if not ((q > -2147483648.0) & (q < 2147483648.0)).all():
        raise ValueError("a position is outside what an int holds")
    return numpy.trunc(q).astype(numpy.int64)


def last_of_each_pair(n, rows, cols):
    """(lo, hi, k): the unordered pairs lo < hi the entries name and the index k of the LAST entry
    of each; diagonal entries are skipped, a bin outside [0, n) is a ValueError."""
    r, c = numpy.asarray(rows, dtype=numpy.int64), numpy.asarray(cols, dtype=numpy.int64)
    lo, hi = numpy.minimum(r, c), numpy.maximum(r, c)
    off = numpy.flatnonzero(lo != hi)
    if off.size and (lo[off].min() < 0 or hi[off].max() >= n):
        raise ValueError("a bin is outside the map")
    key = lo[off] * n + hi[off]
    order = numpy.argsort(key, kind="stable")           # equal keys stay in entry order
    ks = key[order]
    last = order[numpy.append(ks[1:] != ks[:-1], True)] if ks.size else order
    k = off[last]
    return lo[k], hi[k], k


def _kr_quotient(v, lo, hi, kr, ke):
    with numpy.errstate(all="ignore"):
        return nan_to_num(v / (kr[lo] * kr[hi] * ke[hi - lo]))


def _pad(v, n):
    """A KR vector shorter than the map: the missing bins are NaN (no constraint)."""
    out = numpy.full(n, numpy.nan)
    out[:len(v)] = v
    return out


def matrix_of(route, n, dtype, kind="wish", alpha=3.0, **inp):
    """The symmetric (n, n) float64 matrix of the wish distances a route must leave in the
    units of a `dtype` solver.  route and its inputs:
      'dense'    matrix
      'entries'  rows, cols, vals [, kr, ke]
      'triples'  triples (m, 3) [pos_i, pos_j, count], resolution [, kr, ke]
      'coords'   xs (n, 3)"""
    if route == "dense":
        m = numpy.asarray(inp["matrix"], dtype=numpy.float64)
        assert m.shape == (n, n)
        u = numpy.triu(wish_from_value(m, kind, alpha, dtype), 1)
        return u + u.T
    if route == "coords":
        u = numpy.triu(flush_wish(sm.pair_distances(inp["xs"]), dtype), 1)
        return u + u.T
    if route == "triples":
        t = numpy.asarray(inp["triples"], dtype=numpy.float64)
        rows, cols = bins_of(t[:, 0], inp["resolution"]), bins_of(t[:, 1], inp["resolution"])
        vals = nan_to_num(t[:, 2])
    elif route == "entries":
        rows, cols, vals = inp["rows"], inp["cols"], numpy.asarray(inp["vals"], dtype=numpy.float64)
    else:
        raise ValueError(route)
    lo, hi, k = last_of_each_pair(n, rows, cols)
    v = vals[k]
    if inp.get("kr") is not None:
        v = _kr_quotient(v, lo, hi, _pad(inp["kr"], n), _pad(inp["ke"], n))
    w = numpy.zeros((n, n))
    w[lo, hi] = wish_from_value(v, kind, alpha, dtype)
    return w + w.T


def matrix_by_assignment(n, rows, cols, vals, dtype, kind="wish", alpha=3.0):
    """The 'entries' rule (no KR) by numpy assignment in entry order: every entry is converted
    and stored, a later one over an earlier one.  (numpy leaves the order of a fancy assignment
    with repeated indices open; with contiguous index arrays it is the entries' order, which
    tests/test_input_model_cpu.py holds against a Python loop and against last_of_each_pair.)"""
    r, c = numpy.asarray(rows, dtype=numpy.int64), numpy.asarray(cols, dtype=numpy.int64)
    lo, hi = numpy.minimum(r, c), numpy.maximum(r, c)
    off = lo != hi
    flat = numpy.zeros(n * n)
    flat[lo[off] * n + hi[off]] = wish_from_value(numpy.asarray(vals)[off], kind, alpha, dtype)
    w = flat.reshape(n, n)
    return w + w.T


def block_diagonal(n, blocks):
    """The matrix of a solver of several maps: blocks = [(first bin, matrix), ...]."""
    w = numpy.zeros((n, n))
    for a, m in blocks:
        w[a:a + m.shape[0], a:a + m.shape[0]] = m
    return w


# ---- what the probes must return ----------------------------------------------------------------
def degrees_of(w):
    return (w > 0).sum(axis=1).astype(numpy.int64)


def weight_sums_of(w, q):
    """s_i = sum_j w_ij^-q in float64 (numpy's order: exact only where every partial sum is)."""
    with numpy.errstate(all="ignore"):
        t = numpy.where(w > 0, 1.0 / (w if q == 1 else w * w), 0.0)
    return t.sum(axis=1)


def matvec_sq_of(w, x):
    """(w o w) @ x for a map whose entries are multiples of 1/4 and integer x: exact, int64."""
    return sm.matvec_sq_int(4.0 * w, x) / 16.0


def stress_of(w, x, dtype):
    """SPEC 2.3 at the coordinates x: the sum over the constrained pairs i < j of (d_ij - w_ij)^2,
    d_ij = sqrt(|x_i - x_j|^2 + eps^2) (SPEC 2.2), in float64."""
    d = numpy.sqrt(sm.pair_distances(x) ** 2 + (1e-30 if dtype == "float32" else 1e-300))
    on = numpy.triu(w > 0, 1)
    return float(((d - w)[on] ** 2).sum())


def weight_sum_bound(w, q, extra):
    """|device - weight_sums_of| allowed on a float map: (extra + (n + 16) 2^-53) s_i, n the
    pairs of that sum -- each term is rounded once or twice, each of the n - 1 additions once,
    all terms positive; `extra` is what the device's pow may add (SPEC 4)."""
    return (extra + (degrees_of(w) + 16) * 2.0 ** -53) * weight_sums_of(w, q)


# ---- generators ---------------------------------------------------------------------------------
def integer_map(n, seed=0):
    return sm.integer_map(n, seed)


def rhs_blocks(n, seed=0):
    """Two integer right-hand-side blocks in [-2, 2]: six vectors."""
    return sm.integer_rhs(n, seed), sm.integer_rhs(n, seed + 1)


def pow2_map(n, seed=0):
    """A dense symmetric map with wish distances in {0, 1/4, 1/2, 1, 2}: delta^-2 is in
    {0, 16, 4, 1, 1/4} and delta^2 x a multiple of 1/16 -- every sum is exact in float64, and
    below 2^24 sixteenths in float32."""
    u = numpy.triu(POW2[numpy.random.default_rng(seed + 3).integers(0, POW2.size, (n, n))], 1)
    return u + u.T


def pow2_kr(n, seed=0):
    """(kr, ke): every entry 2^k, |k| <= 3; about 3 % of kr and two separations of ke are NaN."""
    rng = numpy.random.default_rng(seed + 9)
    kr = 2.0 ** rng.integers(-3, 4, n)
    ke = 2.0 ** rng.integers(-3, 4, n)
    kr[rng.random(n) < 0.03] = numpy.nan
    ke[[min(7, n - 1), n // 2]] = numpy.nan
    return kr, ke


def line_coords(n, seed=0):
    """x*_i = t_i (1, 2, 2), t_i in 0..3: every distance is 3 |t_i - t_j|, exact; coincident bins
    carry no constraint."""
    t = numpy.random.default_rng(seed + 5).integers(0, 4, n).astype(numpy.float64)
    return t[:, None] * numpy.array([1.0, 2.0, 2.0])


def with_junk(w, seed=0):
    return sm.with_junk(w, seed)


def entries_case(n, seed=0, band=None, kr=None, ke=None, huge=True, most=300000):
    """(rows, cols, vals) whose cleaned values are powers of two: the pairs of a band of
    half-width `band`, or `most` random pairs at the most; 30 % of the pairs named again; the
    whole list in random order, half of it in the lower triangle; a tenth of the bins with a
    diagonal entry.  A value is one of {0, 1/4, 1/2, 1, 2} times the pair's KR denominator
    (1 where that is NaN), so that the quotient is exact.  huge: the last three entries are +inf
    (the largest double after nan_to_num: a distance of 1.8e308 in fp64 -- whose square no
    product holds, see `check` in test_gpu_input_routes -- and no constraint in fp32)."""
    rng = numpy.random.default_rng(seed + 21)
    if band is None:
        m = min(most, n * (n - 1) // 4)
        i, j = rng.integers(0, n, m), rng.integers(0, n, m)
        i, j = i[i != j], j[i != j]
    else:
        i, j, _ = sm.band_entries(n, band, seed)
    again = rng.integers(0, i.size, (3 * i.size) // 10)
    diag = rng.integers(0, n, n // 10 + 1)
    i, j = numpy.concatenate([i, i[again], diag]), numpy.concatenate([j, j[again], diag])
    order = rng.permutation(i.size)
    i, j = i[order], j[order]
    flip = rng.random(i.size) < 0.5
    rows, cols = numpy.where(flip, j, i).astype(numpy.int64), numpy.where(flip, i, j).astype(numpy.int64)
    vals = POW2[rng.integers(0, POW2.size, rows.size)]
    if kr is not None:
        lo, hi = numpy.minimum(rows, cols), numpy.maximum(rows, cols)
        den = kr[lo] * kr[hi] * ke[hi - lo]
        vals = vals * numpy.where(numpy.isfinite(den), den, 1.0)
    if huge:
        off = numpy.flatnonzero(rows != cols)[-3:]
        rows = numpy.concatenate([rows, rows[off]])
        cols = numpy.concatenate([cols, cols[off]])
        vals = numpy.concatenate([vals, [numpy.inf] * 3])
    return rows, cols, vals


def triples_of(rows, cols, vals, resolution=RESOLUTION, seed=0):
    """The entries as Rao-format triples whose positions lie anywhere inside their bin: at its
    start, at bin * res + res - 1, in between (fractions included); for bin 0 also in (-res, 0)
    and NaN.  A twentieth of the counts that are 0 become NaN or -inf."""
    rng = numpy.random.default_rng(seed + 33)

    def positions(b):
        where = rng.integers(0, 4, b.size)
        inside = numpy.select([where == 0, where == 1, where == 2],
                              [0.0, resolution - 1.0, rng.integers(0, resolution, b.size)],
                              rng.random(b.size) * (resolution - 1))
        p = b * float(resolution) + inside
        zero = numpy.flatnonzero(b == 0)
        pick = rng.integers(0, 4, zero.size)
        p[zero[pick == 1]] = -(resolution - 1.0)
        p[zero[pick == 2]] = -0.5
        p[zero[pick == 3]] = numpy.nan
        return p

    t = numpy.column_stack([positions(rows), positions(cols), vals])
    none = numpy.flatnonzero(t[:, 2] == 0.0)
    none = none[rng.random(none.size) < 0.05]
    t[none, 2] = numpy.where(rng.random(none.size) < 0.5, numpy.nan, -numpy.inf)
    return t


def hic_like_counts(n, seed):
    """c_ij ~ Poisson(200 |i - j|^-1.08), 2 % dead bins -- the map of
    tests/test_gpu_shortest_paths.py."""
    r = numpy.random.default_rng(seed)
    i = numpy.arange(n)
    sep = numpy.abs(i[:, None] - i[None, :]).astype(numpy.float64)
    lam = 200.0 * numpy.maximum(sep, 1.0) ** -1.08
    numpy.fill_diagonal(lam, 0.0)
    c = numpy.triu(r.poisson(lam), 1).astype(numpy.float64)
    dead = r.random(n) < 0.02
    c[dead, :] = 0.0
    c[:, dead] = 0.0
    return c


def float_case(n, seed=0):
    """(triples, kr, ke) of the float-map case on n bins (the ContactMap's edge: its n_bins is
    n - 1 and no triple names its last, padding bin): the stored counts of hic_like_counts in
    random order, positions on the grid, KR vectors with NaNs, and one infinite count on a pair
    whose KR denominator is below 1 -- its quotient overflows to the largest double."""
    nb = n - 1
    rng = numpy.random.default_rng(seed + 41)
    c = hic_like_counts(nb, seed)
    i, j = numpy.nonzero(c)
    order = rng.permutation(i.size)
    i, j = i[order], j[order]
    kr = rng.uniform(0.5, 2.0, nb)
    kr[rng.random(nb) < 0.02] = numpy.nan
    ke = rng.uniform(0.5, 2.0, nb) * (numpy.arange(nb) + 1.0) ** -1.08
    ke[nb // 3] = numpy.nan
    den = kr[i] * kr[j] * ke[j - i]
    v = c[i, j].copy()
    v[numpy.flatnonzero(den < 1.0)[0]] = numpy.inf
    return numpy.column_stack([i * float(RESOLUTION), j * float(RESOLUTION), v]), kr, ke


# ---- the cases -----------------------------------------------------------------------------------
# (dtype, n) -> (vw, rows per unit): the smallest sizes that keep the layouts' edges -- a ragged
# strip and three strips plus one column (fp32), one and several strips of the narrow fp64
# layout, the wide fp64 layout (from 4,097 bins on)
LAYOUTS = {("float32", 700): (512, 4), ("float32", 1537): (512, 4),
           ("float64", 300): (128, 8), ("float64", 1300): (128, 8), ("float64", 4097): (512, 2),
           ("float32", 300): (512, 4),                       # (the rank-share case whose last rank is empty)
           ("float32", 1300): (512, 4)}                      # (the chunk-seam case, with float64 1,300)
CASES = tuple(LAYOUTS)[:5]
SMALL = tuple(c for c in CASES if c[1] <= 4096)              # the row-owner path's sizes
BAND = 200                                                   # half-width of the blocked-sparse cases
SEAM_CHUNK = 1 << 22                                         # set_wish_sparse stages this many entries
SEAM_BINS = 1300
MANY = {"float32": ((700, 512, 130), (0, 1024, 1536)), "float64": ((300, 128, 129), (0, 384, 512))}
FLOAT_CASES = (("float32", 1537), ("float64", 1300), ("float64", 4097))


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def rhs(n):
    return _frozen(*rhs_blocks(n, seed=n))


@functools.lru_cache(maxsize=4)
def dense_case(n, which="pow2"):
    """(clean map, the same with junk): 'pow2' or 'integer'."""
    w = pow2_map(n, seed=n) if which == "pow2" else integer_map(n, seed=n)
    return _frozen(w, with_junk(w, seed=n))


@functools.lru_cache(maxsize=None)
def kr_case(n):
    return _frozen(*pow2_kr(n, seed=n))


@functools.lru_cache(maxsize=8)
def sparse_case(n, band, with_kr, huge=True):
    """(rows, cols, vals, kr, ke) of the entry routes: band None (dense tile list) or BAND."""
    kr, ke = kr_case(n) if with_kr else (None, None)
    return _frozen(*entries_case(n, seed=n, band=band, kr=kr, ke=ke, huge=huge)) + (kr, ke)


@functools.lru_cache(maxsize=8)
def triples_case(n, band, with_kr, huge=True):
    rows, cols, vals, kr, ke = sparse_case(n, band, with_kr, huge)
    return _frozen(triples_of(rows, cols, vals, seed=n)) + (kr, ke)


@functools.lru_cache(maxsize=None)
def coords_case(n):
    return _frozen(line_coords(n, seed=n))[0]


def seam_case():
    """(rows, cols, vals, marks) of the chunk-seam case: SEAM_CHUNK + 100,000 entries over
    SEAM_BINS bins.  Chunk 0 draws its pairs from the bins 4 .. 1,299 and chunk 1 from
    100 .. 1,299: the pairs with a bin in 4 .. 99 are named in chunk 0 only, most of the others
    in both.  The bins 0 .. 3 hold the marked pairs: (0, 1) early in chunk 0 and again as its
    FINAL entry; (0, 2) as the FIRST entry of chunk 1 only; (0, 3) in chunk 0 and, with an
    explicit 0, in chunk 1; (1, 2) in chunk 0 only."""
    n, c = SEAM_BINS, SEAM_CHUNK
    m = c + 100000
    rng = numpy.random.default_rng(7)
    first = numpy.where(numpy.arange(m) < c, 4, 100)
    rows = first + (rng.random(m) * (n - first)).astype(numpy.int64)
    cols = first + (rng.random(m) * (n - first)).astype(numpy.int64)
    vals = POW2[rng.integers(0, POW2.size, m)]
    marks = {"final of chunk 0": (c - 1, 0, 1, 2.0), "early in chunk 0": (5, 1, 0, 0.5),
             "first of chunk 1": (c, 2, 0, 0.25), "chunk 0, loses": (9, 0, 3, 1.0),
             "chunk 1, explicit 0": (c + 50000, 3, 0, 0.0), "chunk 0 only": (11, 1, 2, 0.5)}
    for k, r, q, v in marks.values():
        rows[k], cols[k], vals[k] = r, q, v
    return rows, cols, vals, marks


def many_case(dtype, seed=0):
    """(total bins, offsets, maps, tiles) of the solver of three maps on the maps' own dense
    triangles; tiles in device order (J, then I)."""
    edges, offsets = MANY[dtype]
    vw = 512 if dtype == "float32" else 128
    total = offsets[-1] + edges[-1]
    maps = [pow2_map(e, seed=seed + 100 * q + e) for q, e in enumerate(edges)]
    ti, tj = [], []
    for a, e in zip(offsets, edges):
        b0, b1 = a // vw, (a + e + vw - 1) // vw
        for J in range(b0, b1):
            for I in range(b0, J + 1):
                ti.append(I)
                tj.append(J)
    return total, offsets, maps, (numpy.array(ti, dtype=numpy.int32), numpy.array(tj, dtype=numpy.int32))


def sixteenths_exact(w, x):
    """The exactness precondition of a power-of-two case: every entry of w a multiple of 1/4
    (so w^2 x is one of 1/16), no partial sum of the product reaching 2^24 sixteenths (float32
    holds each), and the weighted sums w^-2 multiples of 1/16 below 2^53."""
    fin = numpy.where(w < 1e150, w, 0.0)                  # (the 1.8e308 cells are compared apart)
    s = weight_sums_of(fin, 2)
    return (numpy.array_equal(4.0 * fin, numpy.round(4.0 * fin))
            and sm.largest_partial_sum(4.0 * fin, x) < sm.MAX_EXACT
            and numpy.array_equal(16.0 * s, numpy.round(16.0 * s)) and float(s.max()) * 16.0 < 2.0 ** 53)
