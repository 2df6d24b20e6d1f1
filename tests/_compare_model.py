"""Float64 model of SPEC 2.10 (bb_structures_moments / bb_structures_compare,
compare_structures) in numpy.  Test-only.

Every term is computed as SPEC 2.10 writes it (differences, products and sums rounded one by one,
correctly rounded roots) and summed in extended precision, so the model's own summation error is
far below one float64 ulp of a sum; the aligned copy, the per-bin deviation and every pair
distance are the device's bits.  The bounds are built as tests/_score_model.sums_and_bounds builds
its own: the number of terms times 2^-53 times the sum of the terms' magnitudes, plus the
roundings of a term itself.  On the inputs of exact_case() every term and every sum is an integer
below 2^53 and the model is exact; so are the 18 moments on those of exact_moments_case().
pair_sums lists all pairs (1.3 GB at n = 4,097); pair_sums_by_diagonal gives the same bits from
O(n) memory, for the sizes above that."""
import numpy
import scipy.stats

from tests._score_model import _segment_sums

EPS = 2.0 ** -53
TILE = 256                      # the tile edge of the pair pass (kT of bb_compare.hip)
SORT_TILE = 4096                # slots per workgroup of the device's sort (bb_sort.hip)


def used_bins(A, B, mask=None):
    used = numpy.isfinite(A).all(axis=1) & numpy.isfinite(B).all(axis=1)
    return used if mask is None else used & numpy.asarray(mask, dtype=bool)


def _wide_sum(x, axis=0):
    return numpy.asarray(x, dtype=numpy.longdouble).sum(axis=axis)


def moments_and_bounds(A, B, used):
    """(out18, bound18) of bb_structures_moments: n_used, cA, cB, EA, EB, H row-major.  The
    centred sums are taken about the model's own float64 means; the device's means may differ
    from them by the means' bound, which moves a centred term by its derivative times that."""
    a, b = A[used], B[used]
    nu = a.shape[0]
    out, bound = numpy.zeros(18), numpy.zeros(18)
    out[0] = nu
    mean, mean_bound = numpy.zeros(6), numpy.zeros(6)
    for q, col in enumerate([a[:, 0], a[:, 1], a[:, 2], b[:, 0], b[:, 1], b[:, 2]]):
        mean[q] = float(_wide_sum(col) / nu)
        mean_bound[q] = (nu + 2) * EPS * float(_wide_sum(numpy.abs(col))) / nu     # the sum, the quotient
    out[1:7], bound[1:7] = mean, mean_bound
    da, db = a - mean[:3], b - mean[3:]
    ada, adb = numpy.abs(da), numpy.abs(db)
    for slot, d, ad, mb in ((7, da, ada, mean_bound[:3]), (8, db, adb, mean_bound[3:])):
        terms = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        out[slot] = float(_wide_sum(terms))
        # a term: 3 differences, 3 products, 2 sums; d (x - c)^2 / dc = 2 |x - c|
        bound[slot] = ((nu + 8) * EPS * out[slot] + 2.0 * float((_wide_sum(ad) * mb).sum())
                       + nu * float((mb * mb).sum()))
    for p in range(3):
        for q in range(3):
            out[9 + 3 * p + q] = float(_wide_sum(db[:, p] * da[:, q]))
            mag = float(_wide_sum(adb[:, p] * ada[:, q]))
            bound[9 + 3 * p + q] = ((nu + 4) * EPS * mag + float(_wide_sum(adb[:, p])) * mean_bound[q]
                                    + float(_wide_sum(ada[:, q])) * mean_bound[3 + p]
                                    + nu * mean_bound[q] * mean_bound[3 + p])
    return out, bound


def transform(A, B, used, R, t, s):
    """(aligned, dev2): the device's bits.  aligned_i = ((R[p][0] x + R[p][1] y) + R[p][2] z) s +
    t[p], dev2_i = (ex^2 + ey^2) + ez^2 of e = A_i - aligned_i; NaN at unused bins."""
    R, t = numpy.asarray(R, dtype=numpy.float64).reshape(3, 3), numpy.asarray(t, dtype=numpy.float64)
    x, y, z = B[:, 0], B[:, 1], B[:, 2]
    with numpy.errstate(invalid="ignore", over="ignore"):
        al = numpy.stack([((R[p, 0] * x + R[p, 1] * y) + R[p, 2] * z) * float(s) + t[p] for p in range(3)], axis=1)
        e = A - al
        dev2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
    al[~used], dev2[~used] = numpy.nan, numpy.nan
    return al, dev2


def _distance(x, i, j):
    dx, dy, dz = (x[i, c] - x[j, c] for c in range(3))
    return numpy.sqrt((dx * dx + dy * dy) + dz * dz)


def pairs_of(used):
    """(i, j): the pairs i < j of used bins in canonical order (by i, then j), original indices."""
    idx = numpy.nonzero(used)[0]
    u, v = numpy.triu_indices(idx.shape[0], 1)
    return idx[u], idx[v]


def pair_sums(A, aligned, used, with_magnitudes=False):
    """(profile (n, 7), bins (n, 2)) of SPEC 2.10; with_magnitudes: also the same arrays with
    (dA + dB)^2 for (dA - dB)^2, the magnitude B the bound of that column is stated in (the
    others are their own)."""
    n = A.shape[0]
    i, j = pairs_of(used)
    da, db = _distance(A, i, j), _distance(aligned, i, j)
    k = j - i
    by_k, by_j = numpy.argsort(k, kind="stable"), numpy.argsort(j, kind="stable")
    k_sorted, j_sorted = k[by_k], j[by_j]

    def sums(terms, cols):
        profile, bins = numpy.zeros((n, 7)), numpy.zeros((n, 2))
        for col, t in zip(cols, terms):
            profile[:, col] = _segment_sums(t[by_k], k_sorted, n)
            if col in (0, 6):
                bins[:, (0, 6).index(col)] = _segment_sums(t, i, n) + _segment_sums(t[by_j], j_sorted, n)
        return profile, bins

    res = da - db
    profile, bins = sums([numpy.ones_like(da), da, db, da * da, db * db, da * db, res * res], range(7))
    if not with_magnitudes:
        return profile, bins
    tot = da + db
    mag_profile, mag_bins = sums([numpy.ones_like(da), tot * tot], (0, 6))
    mag_profile[:, 1:6] = profile[:, 1:6]
    return profile, bins, mag_profile, mag_bins


def pair_sums_and_bounds(A, aligned, used):
    """(profile, bins, profile_bound, bins_bound): |device - model| allowed per entry is
    (pairs + 16) 2^-53 B: each term is within 8 * 2^-53 of its B-term on either side (the
    distances themselves are the device's bits), and a float64 sum of non-negative terms in any
    order within their number times 2^-53."""
    p, b, mp, mb = pair_sums(A, aligned, used, with_magnitudes=True)
    return p, b, (p[:, :1] + 16) * EPS * mp, (b[:, :1] + 16) * EPS * mb


def _one_segment(terms):
    """The float64 that _segment_sums gives the terms (..., m) as one segment each: the same
    numpy call on the same numbers in the same order, hence the same bits (add.reduceat adds a
    segment's first term to the pairwise sum of the rest wherever the segment starts, which a
    plain .sum() does not; tests/test_compare_cpu.py holds the two routes against each other)."""
    if terms.shape[-1] == 0:
        return numpy.zeros(terms.shape[:-1])
    return numpy.add.reduceat(terms.astype(numpy.longdouble), [0], axis=-1)[..., 0].astype(numpy.float64)


def pair_sums_by_diagonal(A, aligned, used, with_magnitudes=False):
    """pair_sums without the list of all pairs: the same arrays and the same bits in O(n)
    memory and O(n^2) time (0.9 s at n = 4,097 where pair_sums takes 3.6 s, 3 s at 8,193).  The
    terms are formed as _distance and pair_sums form them and summed in numpy.longdouble, a
    segment of pair_sums at a time:
      the profile  walks the separations k = 1 .. n - 1 over the slices x[:-k], x[k:]: the used
                   pairs of one k by ascending i are pair_sums' segment of k;
      the bins     walk the used bins i over x[i] against x: the used j > i and the used j < i,
                   each by ascending j, are pair_sums' two segments of bin i (a pair's terms are
                   the same bits from either end: (-d)^2 = d^2)."""
    n = A.shape[0]
    used = numpy.asarray(used, dtype=bool)
    every = bool(used.all())
    x = numpy.ascontiguousarray(numpy.stack([numpy.asarray(A, dtype=numpy.float64).T,
                                             numpy.asarray(aligned, dtype=numpy.float64).T]))   # (2, 3, n)
    x[:, :, ~used] = 0.0                                            # (finite; never in a sum)
    profile, bins = numpy.zeros((n, 7)), numpy.zeros((n, 2))
    mag_profile, mag_bins = numpy.zeros((n, 7)), numpy.zeros((n, 2))

    def distances(d):
        d *= d
        return numpy.sqrt((d[:, 0] + d[:, 1]) + d[:, 2])

    def squares(da, db):                                            # (dA - dB)^2 and, where asked, (dA + dB)^2
        sq = numpy.stack([da - db, da + db]) if with_magnitudes else (da - db)[None]
        sq *= sq
        return sq

    def separation(k):
        m = n - k
        on = None if every else used[:m] & used[k:]
        if on is not None and not on.any():
            return
        dist = distances(x[:, :, :m] - x[:, :, k:])
        if on is not None:
            dist = dist[:, on]
        da, db = dist
        sq = squares(da, db)
        profile[k, 0] = da.shape[0]
        profile[k, 1:] = _one_segment(numpy.stack([da, db, da * da, db * db, da * db, sq[0]]))
        if with_magnitudes:
            mag_profile[k, 6] = _one_segment(sq[1])

    def one_bin(i):
        da, db = distances(x[:, :, i:i + 1] - x)
        sq = squares(da, db)
        below, above = sq[:, :i], sq[:, i + 1:]
        if not every:
            below, above = below[:, used[:i]], above[:, used[i + 1:]]
        total = _one_segment(above) + _one_segment(below)
        bins[i] = below.shape[1] + above.shape[1], total[0]
        if with_magnitudes:
            mag_bins[i] = bins[i, 0], total[1]

    for k in range(1, n):
        separation(k)
    for i in numpy.nonzero(used)[0]:
        one_bin(i)
    if not with_magnitudes:
        return profile, bins
    mag_profile[:, :6] = profile[:, :6]
    return profile, bins, mag_profile, mag_bins


def pair_sums_and_bounds_by_diagonal(A, aligned, used):
    """pair_sums_and_bounds through pair_sums_by_diagonal: the same rule."""
    p, b, mp, mb = pair_sums_by_diagonal(A, aligned, used, with_magnitudes=True)
    return p, b, (p[:, :1] + 16) * EPS * mp, (b[:, :1] + 16) * EPS * mb


def centred_ranks(d):
    """scipy's average ranks of d less (m + 1) / 2: exact half-integers."""
    return scipy.stats.rankdata(d) - (d.shape[0] + 1) / 2.0


def rank_sums_and_bounds(A, aligned, used):
    """(sums4, bound4): m, sum rA^2, sum rB^2, sum rA rB.  The ranks are exact; a product is
    rounded once and a float64 sum of m terms in any order is within m 2^-53 of the sum of their
    magnitudes."""
    i, j = pairs_of(used)
    m = i.shape[0]
    if m == 0:
        return numpy.zeros(4), numpy.zeros(4)
    ra = centred_ranks(_distance(A, i, j)).astype(numpy.longdouble)
    rb = centred_ranks(_distance(aligned, i, j)).astype(numpy.longdouble)
    out = numpy.array([m, float((ra * ra).sum()), float((rb * rb).sum()), float((ra * rb).sum())])
    mag = numpy.array([0.0, out[1], out[2], float(numpy.abs(ra * rb).sum())])
    return out, (m + 2) * EPS * mag


def spearman(sums4):
    """rho from the four numbers, by SPEC 2.10's rule."""
    m, raa, rbb, rab = (float(v) for v in sums4)
    return rab / numpy.sqrt(raa * rbb) if m >= 2 and raa > 0 and rbb > 0 else numpy.nan


def spearman_bound(sums4, bound4):
    """|rho(device sums) - rho(model sums)| allowed: the sums' bounds through
    rho = Sab / sqrt(Saa Sbb), and 4 roundings of the host's own arithmetic."""
    m, raa, rbb, rab = (float(v) for v in sums4)
    root = numpy.sqrt(raa * rbb)
    return bound4[3] / root + abs(rab / root) * 0.5 * (bound4[1] / raa + bound4[2] / rbb) * 1.01 + 4 * EPS


def superposition(mo, mirror=True, scale=False):
    """(R, t, s, mirrored) from the 18 moments, straight from SPEC 2.10: both candidates are
    formed and the one with the smaller residual EA + s^2 EB - 2 s tr(S D) is taken."""
    mo = numpy.asarray(mo, dtype=numpy.float64)
    c_a, c_b, e_a, e_b, H = mo[1:4], mo[4:7], mo[7], mo[8], mo[9:].reshape(3, 3)
    U, S, Vt = numpy.linalg.svd(H)
    det = numpy.sign(numpy.linalg.det(Vt.T @ U.T)) or 1.0
    best = None
    for last in ((det, -det) if mirror else (det,)):
        D = numpy.array([1.0, 1.0, last])
        tr = float((S * D).sum())
        s = tr / e_b if scale else 1.0
        res = e_a + s * s * e_b - 2 * s * tr
        if best is None or res < best[0]:
            R = (Vt.T * D) @ U.T
            best = (res, R, c_a - s * (R @ c_b), s, last != det)
    return best[1:]


# ---- the cases ------------------------------------------------------------------------------------
def exact_case(n, seed=0):
    """A_i = (a_i, 0, 0), B_i = (0, b_i, 0) with a, b integers in [0, 1000): under the identity
    transform every distance, product and sum is an integer below 2^53."""
    rng = numpy.random.default_rng(2100 + 13 * n + seed)
    A, B = numpy.zeros((n, 3)), numpy.zeros((n, 3))
    A[:, 0] = rng.integers(0, 1000, n)
    B[:, 1] = rng.integers(0, 1000, n)
    return A, B


def edge_mask(n, tile=TILE, seed=0):
    """Drops the first and the last bin, both bins across every tile boundary and a seeded
    tenth of the rest."""
    mask = numpy.random.default_rng(77 + n + seed).random(n) >= 0.1
    mask[0] = mask[n - 1] = False
    for edge in range(tile, n, tile):
        mask[edge - 1] = mask[edge] = False
    return mask


def block_mask(n, tile=TILE, seed=0, blocks=((768, 1024), (1024, 2048))):
    """edge_mask less whole blocks of bins [begin, end): by default one tile of the pair pass
    (768 .. 1,023) and the four after it (1,024 .. 2,047), which are a whole workgroup of the
    moment kernels (kMomentBins = 1,024) and, from n = 4,097 on, every tile of one chunk of the
    pair pass on the main tile diagonal."""
    mask = edge_mask(n, tile, seed)
    for begin, end in blocks:
        mask[begin:end] = False
    return mask


def exact_moments_case(n, used, seed=0):
    """(A, B): integers in [0, 1000) in all six columns, the last used bin then raised (by less
    than n_used) so that every column's sum over the used bins is a multiple of n_used.  The
    means are then integers, and so is every centred term and every one of the 18 moments, all
    below 2^53: exact in float64 in whatever order they are added."""
    rng = numpy.random.default_rng(4200 + 7 * n + seed)
    A = rng.integers(0, 1000, (n, 3)).astype(numpy.float64)
    B = rng.integers(0, 1000, (n, 3)).astype(numpy.float64)
    idx = numpy.nonzero(used)[0]
    nu = idx.shape[0]
    for x in (A, B):
        x[idx[-1]] += (-x[idx].sum(axis=0)) % nu
    return A, B


IDENTITY13 = numpy.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1])


def rotation(seed):
    """A proper rotation, seeded."""
    q, _ = numpy.linalg.qr(numpy.random.default_rng(seed).standard_normal((3, 3)))
    return q * numpy.sign(numpy.linalg.det(q))


def similarity_image(A, seed=3, mirrored=True, scale=0.37, noise=0.0):
    """B with A_i = scale' R' B_i + t' (+ noise): B = scale * R A + t, R a rotation times a
    mirror where asked."""
    R = rotation(seed)
    if mirrored:
        R = R @ numpy.diag([1.0, 1.0, -1.0])
    rng = numpy.random.default_rng(seed + 1)
    B = scale * (A @ R.T) + rng.standard_normal(3) * 5.0
    return B + noise * rng.standard_normal(A.shape) if noise else B


def float_case(n, seed=0):
    """(A, B): a seeded random walk and a noisy, rotated, mirrored and scaled copy of it."""
    from tests import _oracle
    A = _oracle.random_walk(n, seed=seed)
    return A, similarity_image(A, seed=11 + seed, mirrored=True, scale=0.37, noise=0.05)


def integer_case(n, seed=0):
    """(A, B) with integer coordinates, so that ties among the pair distances are plentiful and
    stay ties under any rounding of the root: a walk rounded to a coarse grid and a noisy copy."""
    from tests import _oracle
    walk = _oracle.random_walk(n, seed=seed)
    A = numpy.rint(walk * 0.7)
    B = numpy.rint(walk * 0.7 + numpy.random.default_rng(5 + seed).standard_normal((n, 3)))
    return A, B
