"""Structure against structure (docs/SPEC.md 2.10): the two O(1) / O(n) host steps of a
comparison -- the used-bin vector and the 3 x 3 SVD of the superposition -- around the two device
calls that do the rest (`bb_structures_moments`, `bb_structures_compare`)."""
import numpy

from . import _lib

# the places of a pair are 32 bits wide on the device, so the C entry refuses 2^32 pairs or more;
# the documented limit here is floor(sqrt(2^33)) bins, one below the last count that would fit
MAX_SPEARMAN_BINS = 92681


def superposition(moments, mirror=True, scale=False):
    """(rotation, translation, scale, mirrored) with A_i ~ scale * rotation @ B_i + translation
    from the 18 moments of `bb_structures_moments` (n_used, cA, cB, EA, EB, H row-major with
    H[p][q] = sum (B - cB)_p (A - cA)_q): Kabsch's rotation V diag(1, 1, det) U^T of H = U S V^T,
    or, where `mirror` allows it and its residual is smaller, the improper one, which flips the
    smallest singular direction; scale = tr(S D) / EB where asked for, else 1."""
    mo = numpy.asarray(moments, dtype=numpy.float64).reshape(18)
    c_a, c_b, e_b, H = mo[1:4], mo[4:7], float(mo[8]), mo[9:18].reshape(3, 3)
    U, S, Vt = numpy.linalg.svd(H)
    det = 1.0 if numpy.linalg.det(Vt.T @ U.T) >= 0 else -1.0
    # the residual falls as tr(S D) grows, and S[2] >= 0 is the smallest: D = diag(1, 1, +1) is
    # never worse, and is the improper rotation exactly when det < 0.  A flat structure is its own
    # mirror image (S[2] = 0 to the rounding of the SVD, a tie): the proper rotation.
    last = 1.0 if (mirror and S[2] > 16 * 2.0 ** -53 * S[0]) else det
    D = numpy.array([1.0, 1.0, last])
    R = (Vt.T * D) @ U.T
    s = float((S * D).sum() / e_b) if (scale and e_b > 0) else 1.0
    return R, c_a - s * (R @ c_b), s, bool(last * det < 0)


class StructureComparison(object):
    """Two structures laid on top of each other, from the device's sums (SPEC 2.10,
    `compare_structures`).

    used, n_used : the bins that took part (bool per bin) and how many
    rotation (3, 3), translation (3), scale, mirrored : A_i ~ scale * rotation @ B_i + translation;
        mirrored = the rotation is improper (det -1)
    aligned : (n, 3), B laid onto A (NaN at unused bins)
    bin_sq_deviation : (n,) |A_i - aligned_i|^2 from the device (NaN at unused bins)
    sums : (n, 7) float64, row k = the pairs of used bins of separation j - i = k: pairs, sum dA,
        sum dB, sum dA^2, sum dB^2, sum dA dB, sum (dA - dB)^2 with dA = |A_i - A_j| and
        dB = |aligned_i - aligned_j|
    bin_sums : (n, 2) float64, row i = the pairs that hold bin i: pairs, sum (dA - dB)^2
    rank_sums : None, or m, sum rA^2, sum rB^2, sum rA rB of the centred average ranks

    Derived on the host in float64:
    rmsd, deviation : sqrt(mean |A_i - aligned_i|^2) over the used bins, and |A_i - aligned_i| per bin
    n_pairs, distance_rmsd : the pairs, and sqrt(sum (dA - dB)^2 / n_pairs)
    distance_pearson : Pearson r of (dA, dB); NaN with fewer than 2 pairs or no variance
    distance_spearman : Spearman rho of (dA, dB); NaN unless asked for, with fewer than 2 pairs or
        with no variance in either ranking
    pairs, mean_distance_a, mean_distance_b, rms_difference : per separation k (int64; the others
        NaN where pairs == 0)
    bin_pairs, bin_distance_error : per bin: its pairs (int64) and its sum (dA - dB)^2 (every pair
        counts at both of its bins: the bins add up to twice the total)
    """

    def __init__(self, used, rotation, translation, scale, mirrored, aligned, bin_sq_deviation, sums,
                 bin_sums, rank_sums=None):
        self.used = numpy.asarray(used, dtype=bool)
        n = self.used.shape[0]
        self.n_used = int(self.used.sum())
        self.rotation = numpy.asarray(rotation, dtype=numpy.float64).reshape(3, 3)
        self.translation = numpy.asarray(translation, dtype=numpy.float64).reshape(3)
        self.scale, self.mirrored = float(scale), bool(mirrored)
        self.aligned = numpy.asarray(aligned, dtype=numpy.float64)
        self.bin_sq_deviation = numpy.asarray(bin_sq_deviation, dtype=numpy.float64)
        self.sums = numpy.ascontiguousarray(sums, dtype=numpy.float64)
        self.bin_sums = numpy.ascontiguousarray(bin_sums, dtype=numpy.float64)
        if (self.sums.shape != (n, 7) or self.bin_sums.shape != (n, 2) or self.aligned.shape != (n, 3)
                or self.bin_sq_deviation.shape != (n,)):
            raise ValueError("StructureComparison: sums must be (n, 7), bin_sums (n, 2), aligned (n, 3) "
                             "and bin_sq_deviation (n,)")
        self.rank_sums = None if rank_sums is None else numpy.asarray(rank_sums, dtype=numpy.float64).reshape(4)
        self.deviation = numpy.sqrt(self.bin_sq_deviation)
        self.rmsd = (float(numpy.sqrt(self.bin_sq_deviation[self.used].sum() / self.n_used))
                     if self.n_used else float("nan"))
        tot = self.sums.sum(axis=0)
        m, sa, sb, saa, sbb, sab = (float(v) for v in tot[:6])
        self.n_pairs = int(round(m))
        self.distance_rmsd = float(numpy.sqrt(tot[6] / m)) if self.n_pairs else float("nan")
        # FitScore.pearson's guard: a variance the rounding of its own sums could have made is none
        var_a, var_b, noise = m * saa - sa * sa, m * sbb - sb * sb, 8.0 * m * m * 2.0 ** -53
        self.distance_pearson = (float((m * sab - sa * sb) / numpy.sqrt(var_a * var_b))
                                 if self.n_pairs >= 2 and var_a > noise * saa and var_b > noise * sbb
                                 else float("nan"))
        self.distance_spearman = float("nan")
        if self.rank_sums is not None and self.rank_sums[0] >= 2:
            _, raa, rbb, rab = (float(v) for v in self.rank_sums)
            if raa > 0 and rbb > 0:
                self.distance_spearman = float(rab / numpy.sqrt(raa * rbb))

        def per(total, count):
            return numpy.where(count > 0, total / numpy.where(count > 0, count, 1.0), numpy.nan)
        cnt = self.sums[:, 0]
        self.pairs = numpy.rint(cnt).astype(numpy.int64)
        self.mean_distance_a = per(self.sums[:, 1], cnt)
        self.mean_distance_b = per(self.sums[:, 2], cnt)
        self.rms_difference = numpy.sqrt(per(self.sums[:, 6], cnt))
        self.bin_pairs = numpy.rint(self.bin_sums[:, 0]).astype(numpy.int64)
        self.bin_distance_error = self.bin_sums[:, 1].copy()

    def __repr__(self):
        return ("StructureComparison(n_used=%d, rmsd=%.6g, scale=%.6g, mirrored=%s, distance_rmsd=%.6g, "
                "distance_pearson=%.6g, distance_spearman=%.6g)"
                % (self.n_used, self.rmsd, self.scale, self.mirrored, self.distance_rmsd,
                   self.distance_pearson, self.distance_spearman))


def _coords(name, x):
    x = numpy.asarray(x)
    if x.dtype.kind not in "biuf":
        raise ValueError("compare_structures: %s must be real numbers, not dtype %s" % (name, x.dtype))
    if x.ndim != 2 or x.shape[1] != 3:
        raise ValueError("compare_structures: %s must be (n, 3), not %s" % (name, x.shape))
    return numpy.ascontiguousarray(x, dtype=numpy.float64)


def used_bins(A, B, mask=None):
    """The used-bin vector of SPEC 2.10: in the mask (None: every bin) and all six coordinates
    finite."""
    used = numpy.isfinite(A).all(axis=1) & numpy.isfinite(B).all(axis=1)
    if mask is not None:
        mask = numpy.asarray(mask)
        if mask.dtype.kind not in "biu" or mask.shape != (A.shape[0],):
            raise ValueError("compare_structures: mask must be %d booleans" % A.shape[0])
        used &= mask.astype(bool)
    return used


def compare_structures(A, B, mask=None, mirror=True, scale=False, spearman=False, device=None):
    """Compare two structures of the same bins on the device (docs/SPEC.md 2.10): a
    `StructureComparison`.  A fit is defined up to a rotation, a translation and a mirror image,
    so B is first laid onto A over the USED bins -- those in `mask` (None: all) whose six
    coordinates are finite -- by the rotation (or, with `mirror`, whichever of the rotation and
    the improper rotation leaves the smaller residual), translation and, with `scale`, scale that
    minimise sum |A_i - aligned_i|^2; then the pair distances of the two are compared per
    separation, per bin and in total.  `spearman=True` also ranks the two lists of pair distances
    on the device (40 B of device memory per pair; at most 92,681 used bins).  ValueError for
    arrays that are not (n, 3) reals of one n >= 2, fewer than 2 used bins or too many for
    `spearman`, raised before any device call."""
    A, B = _coords("A", A), _coords("B", B)
    if A.shape != B.shape or A.shape[0] < 2:
        raise ValueError("compare_structures: A and B must hold the same n >= 2 bins, not %s and %s"
                         % (A.shape, B.shape))
    n = A.shape[0]
    used = used_bins(A, B, mask)
    n_used = int(used.sum())
    if n_used < 2:
        raise ValueError("compare_structures: fewer than 2 used bins (in the mask, all coordinates finite)")
    if spearman and n_used > MAX_SPEARMAN_BINS:
        raise ValueError("compare_structures: spearman=True takes at most %d used bins (2^32 pairs), not %d"
                         % (MAX_SPEARMAN_BINS, n_used))
    device = 0 if device is None else int(device)
    lib = _lib.load()
    use = numpy.ascontiguousarray(used, dtype=numpy.uint8)
    moments = numpy.zeros(18)
    _lib.check(lib.bb_structures_moments(_lib.as_f64_ptr(A), _lib.as_f64_ptr(B), use.ctypes.data_as(_lib.p_u8), n,
                                         device, _lib.as_f64_ptr(moments)), "bb_structures_moments")
    R, t, s, mirrored = superposition(moments, mirror=mirror, scale=scale)
    transform = numpy.concatenate([R.reshape(9), t, [s]])
    aligned, bin_dev = numpy.zeros((n, 3)), numpy.zeros(n)
    sums, bin_sums = numpy.zeros((n, 7)), numpy.zeros((n, 2))
    rank_sums = numpy.zeros(4) if spearman else None
    _lib.check(lib.bb_structures_compare(_lib.as_f64_ptr(A), _lib.as_f64_ptr(B), use.ctypes.data_as(_lib.p_u8), n,
                                         _lib.as_f64_ptr(transform), _lib.BB_CMP_SPEARMAN if spearman else 0,
                                         device, _lib.as_f64_ptr(aligned), _lib.as_f64_ptr(bin_dev),
                                         _lib.as_f64_ptr(sums), _lib.as_f64_ptr(bin_sums),
                                         _lib.as_f64_ptr(rank_sums) if spearman else None, None),
               "bb_structures_compare")
    return StructureComparison(used, R, t, s, mirrored, aligned, bin_dev, sums, bin_sums, rank_sums)
