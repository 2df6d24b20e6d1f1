"""The host rules of a fit that need neither an engine nor a rank (docs/SPEC.md 2.4, 2.4.1, 2.11):
the layout and the tile lists, the bins' degrees and the step factors made from them, and the
search for the count-to-distance exponent.  Pure numpy over `bb_layout_dense_info`."""
import math

import numpy

from . import _lib

# the C-ABI's codes of a solver's arithmetic type and of what an input holds (`layout_info` reads
# the first, so they live here; the engines and the triples take them from here)
_DTYPES = {"float32": _lib.BB_F32, "float64": _lib.BB_F64}
_KINDS = {"wish": _lib.BB_KIND_WISH, "counts": _lib.BB_KIND_COUNTS}


def layout_info(n_bins, dtype):
    """bb_layout_dense_info as a dict (host-only arithmetic: no GPU needed)."""
    info = _lib.LayoutInfo()
    _lib.check(_lib.load().bb_layout_dense_info(int(n_bins), _DTYPES[dtype], info),
               "bb_layout_dense_info")
    return info.as_dict()


def tiles_from_entries(n_bins, rows, cols, dtype):
    """The (tile_I, tile_J) list -- device order: J ascending, then I -- of the
    tiles that hold at least one entry (rows[k], cols[k]); either triangle."""
    vw = layout_info(n_bins, dtype)["vw"]     # 512, or 128 for small fp64 problems
    r = numpy.asarray(rows, dtype=numpy.int64)
    c = numpy.asarray(cols, dtype=numpy.int64)
    if r.size and (min(r.min(), c.min()) < 0 or max(r.max(), c.max()) >= n_bins):
        raise ValueError("an index is outside [0, n_bins)")
    lo, hi = numpy.minimum(r, c) // vw, numpy.maximum(r, c) // vw
    nb = (int(n_bins) + vw - 1) // vw
    key = numpy.unique(hi * nb + lo)
    return (key % nb).astype(numpy.int32), (key // nb).astype(numpy.int32)


def tiles_from_blocks(n_bins, boundaries, band_bins, dtype):
    """Tile list of a block-sparse genome-wide map (BASELINE config 5; SURVEY.md 8(d):
    a tile is kept "when genomic separation <= band or the tile has any c > 0"): every
    tile that holds a pair of bins of ONE block of `boundaries` -- a chromosome's own
    contacts, where a Hi-C map is populated -- plus every tile that holds a pair of bins
    at most `band_bins` apart whatever the block.  `boundaries` = ascending bin offsets
    [0, ..., n_bins] (blueberry_amd.utils.genome_boundaries).  Replaces the dense
    `(n_bins+1)**2` float64 matrix of the reference (`blueberry/datatypes.pyx:99`: 720 GB
    at 10 kb) for whole-genome maps.  Returns (tile_I, tile_J) in device order and the
    number of stored pairs i < j < n_bins inside those tiles."""
    vw = layout_info(n_bins, dtype)["vw"]
    n = int(n_bins)
    b = numpy.asarray(boundaries, dtype=numpy.int64)
    if b.ndim != 1 or b.size < 2 or b[0] != 0 or b[-1] != n or (numpy.diff(b) < 0).any():
        raise ValueError("boundaries must ascend from 0 to n_bins")
    nb = (n + vw - 1) // vw
    first = numpy.arange(nb, dtype=numpy.int64) * vw
    last = numpy.minimum(first + vw, n) - 1
    blk_lo = numpy.searchsorted(b, first, side="right") - 1     # block of a tile's first bin
    blk_hi = numpy.searchsorted(b, last, side="right") - 1      # ... and of its last bin
    J, I = numpy.meshgrid(numpy.arange(nb), numpy.arange(nb))
    upper = I <= J
    same_block = blk_hi[I] >= blk_lo[J]           # I <= J and blocks are contiguous runs
    near = (J - I - 1) * vw + 1 <= int(band_bins)   # closest pair of bins of the two tiles
    sel = upper & (same_block | near)
    ti, tj = I[sel], J[sel]
    order = numpy.lexsort((ti, tj))
    ti, tj = ti[order].astype(numpy.int32), tj[order].astype(numpy.int32)
    rows = numpy.minimum(vw, n - ti.astype(numpy.int64) * vw)
    cols = numpy.minimum(vw, n - tj.astype(numpy.int64) * vw)
    pairs = int(numpy.where(ti == tj, rows * (rows - 1) // 2, rows * cols).sum())
    return (ti, tj), pairs


def block_degrees(n_bins, tiles, dtype):
    """Per block of the layout: an upper bound on the number of stored partners of its bins
    under a tile list (tiles in the block's row and column, times the tile edge)."""
    vw = layout_info(n_bins, dtype)["vw"]
    nb = (int(n_bins) + vw - 1) // vw
    ti, tj = numpy.asarray(tiles[0]), numpy.asarray(tiles[1])
    deg = numpy.bincount(ti, minlength=nb) + numpy.bincount(tj, minlength=nb)
    deg -= numpy.bincount(ti[ti == tj], minlength=nb)             # a diagonal tile counts once
    return numpy.minimum(int(n_bins), deg * vw).astype(numpy.int64)


def max_degree(n_bins, tiles, dtype):
    """Upper bound on the number of stored partners of any bin under a tile list: the step
    1 / (2 * max_degree) is the one SPEC 2.4 gives a dense map of that many bins."""
    return int(block_degrees(n_bins, tiles, dtype).max())


def block_step_factors(n_bins, tiles, dtype):
    """(lr, scale) of SPEC 2.4.1 for a tile list: lr = 1 / (2 max_degree) and, per block,
    scale[b] = max_degree / degree[b] -- every block takes the step 1 / (2 degree[b]) its own
    number of stored partners allows (a block without tiles keeps the factor 1)."""
    deg = block_degrees(n_bins, tiles, dtype)
    top = int(deg.max()) if deg.size and deg.max() > 0 else int(n_bins)
    return 1.0 / (2.0 * top), numpy.where(deg > 0, top / numpy.maximum(deg, 1), 1.0)


def degree_step_factors(degree):
    """(lr, scale) of SPEC 2.4.1 from the bins' degrees (number of constraining pairs):
    lr = 1 / (2 (D + 1)), D the largest degree, and scale[i] = (D + 1) / (degree[i] + 1), so
    that bin i steps by 1 / (2 (degree[i] + 1)) -- for a complete map of n bins exactly SPEC
    2.4's 1 / (2 n).  scale is None when all bins have the same degree."""
    deg = numpy.asarray(degree, dtype=numpy.int64)
    top = int(deg.max()) if deg.size else 0
    lr = 1.0 / (2.0 * (top + 1))
    if deg.size == 0 or int(deg.min()) == top:
        return lr, None
    return lr, (top + 1.0) / (deg + 1.0)


# fp32 with weight_power > 0: the largest weighted degree accepted (SPEC 2.3.1).  Every
# weight is then <= 2^60, so the smallest wish distance is 2^-30 (q = 2) or 2^-60 (q = 1)
# relative to a unit weight, and the terms and forces stay finite in float32.
_F32_MAX_WEIGHT_SUM = 2.0 ** 60


def weighted_steps(sums, n_bins, dtype, lr, degree_steps):
    """(lr, scale) for weighted stress from the bins' weighted degrees s_i (SPEC 2.4.1):
    lr='auto' is 1 / (2 max s); degree_steps: scale[i] = max s / s_i (1 where s_i = 0), else
    None.  Raises ValueError for a map fp32 cannot weight without overflow, or whose weights
    are not finite."""
    s = numpy.asarray(sums, dtype=numpy.float64)
    top = float(s.max()) if s.size else 0.0
    if not numpy.isfinite(top):
        raise ValueError("weight_power: the weights delta^-q of this map overflow float64")
    if dtype == "float32" and top > _F32_MAX_WEIGHT_SUM:
        raise ValueError("weight_power: the largest weighted degree of this map, %.3g, exceeds "
                         "2^60: float32 would overflow (use dtype='float64' or rescale the wish "
                         "distances)" % top)
    if top <= 0.0:                                    # no constraint at all
        return (1.0 / (2.0 * n_bins) if lr == "auto" else float(lr)), None
    out_lr = 1.0 / (2.0 * top) if lr == "auto" else float(lr)
    if not degree_steps:
        return out_lr, None
    return out_lr, numpy.where(s > 0.0, top / numpy.where(s > 0.0, s, 1.0), 1.0)


# -- the count-to-distance exponent inferred in the fit (SPEC 2.11) -------------------------------
ALPHA_MIN, ALPHA_MAX = 0.25, 16.0      # what a step of the search is clipped to


def _check_alpha(alpha):
    """The constructor's `alpha` normalised: a positive float, or ('auto', alpha0, max_rounds,
    tol) from 'auto' and the tuples that begin with it (defaults 3.0, 8, 1e-3)."""
    if isinstance(alpha, str) or isinstance(alpha, tuple):
        form = (alpha,) if isinstance(alpha, str) else alpha
        if not (1 <= len(form) <= 4 and isinstance(form[0], str) and form[0] == "auto"):
            raise ValueError("alpha must be a positive number, 'auto', ('auto', alpha0), ('auto', "
                             "alpha0, max_rounds) or ('auto', alpha0, max_rounds, tol)")
        def number(v, what):
            if isinstance(v, bool) or not isinstance(v, (int, float, numpy.integer, numpy.floating)):
                raise ValueError("alpha: %s of 'auto' must be a number" % what)
            return float(v)
        alpha0 = number(form[1], "the start alpha0") if len(form) > 1 else 3.0
        rounds = form[2] if len(form) > 2 else 8
        tol = number(form[3], "tol") if len(form) > 3 else 1e-3
        if not (numpy.isfinite(alpha0) and alpha0 > 0):
            raise ValueError("alpha: the start alpha0 of 'auto' must be positive and finite")
        if (isinstance(rounds, bool) or not isinstance(rounds, (int, numpy.integer))
                or not 1 <= int(rounds) <= 64):
            raise ValueError("alpha: max_rounds of 'auto' must be an int in [1, 64]")
        if not (numpy.isfinite(tol) and tol > 0):
            raise ValueError("alpha: tol of 'auto' must be positive and finite")
        return ("auto", alpha0, int(rounds), tol)
    if not float(alpha) > 0:
        raise ValueError("alpha must be positive")
    return float(alpha)


def loglog_totals(profile):
    """The seven sums of SPEC 2.11 over all separations of one rank's (n_bins, 7) profile, added
    in ascending k."""
    p = numpy.asarray(profile, dtype=numpy.float64)
    return numpy.cumsum(p, axis=0)[-1] if p.shape[0] else numpy.zeros(7)


def loglog_slope(totals):
    """(p, a, r_log, mean u, mean v) from the seven totals (pairs, sum u, sum v, sum u^2,
    sum v^2, sum u v, pairs with d = 0): the least-squares line v = a + p u of log fitted
    distance on log wish distance and their correlation (NaN when v does not vary).
    ValueError: fewer than 3 usable pairs, or a var(u) that the rounding of its own sums could
    have made (SPEC 2.8's guard): the map's counts do not vary.  RuntimeError: p <= 0."""
    n, su, sv, suu, svv, suv = (float(t) for t in numpy.asarray(totals, dtype=numpy.float64)[:6])
    if n < 3:
        raise ValueError("alpha='auto': fewer than 3 usable pairs (stored, delta > 0, d > 0): "
                         "no slope to take")
    noise = 8.0 * n * n * 2.0 ** -53
    var_u, var_v = n * suu - su * su, n * svv - sv * sv
    if not var_u > noise * suu:
        raise ValueError("alpha='auto': the wish distances of the stored pairs do not vary (the "
                         "map's counts are all alike): no exponent can be inferred")
    cov = n * suv - su * sv
    p = cov / var_u
    if not p > 0:
        raise RuntimeError("alpha='auto': the log-log slope of fitted on wish distance is %.6g "
                           "<= 0: the fit does not follow the map (more iterations, another "
                           "start or a fixed alpha)" % p)
    r_log = cov / numpy.sqrt(var_u * var_v) if var_v > noise * svv else float("nan")
    ubar, vbar = su / n, sv / n
    return p, vbar - p * ubar, float(r_log), ubar, vbar


def next_alpha(history):
    """The exponent of the next round from history = [(alpha_0, p_0), ..., (alpha_r, p_r)]
    (SPEC 2.11): alpha_r / p_r after the first round; later a secant step on (ln alpha, ln p),
    alpha_r / p_r again when its slope g is not finite and > 0; clipped to [alpha_r / 2,
    2 alpha_r], then to [ALPHA_MIN, ALPHA_MAX]."""
    a1, p1 = (float(v) for v in history[-1][:2])
    nxt = a1 / p1
    if len(history) >= 2:
        a0, p0 = (float(v) for v in history[-2][:2])
        with numpy.errstate(divide="ignore", invalid="ignore"):
            g = numpy.float64(math.log(p1) - math.log(p0)) / numpy.float64(math.log(a1) - math.log(a0))
        if numpy.isfinite(g) and g > 0:
            nxt = math.exp(math.log(a1) - math.log(p1) / float(g))
    nxt = min(max(nxt, a1 / 2.0), 2.0 * a1)
    return min(max(nxt, ALPHA_MIN), ALPHA_MAX)
