"""Inputs and host references shared by the ContactMap-stage tests
(tests/test_gpu_contactmap_stage.py on the device, tests/test_contactmap_stage_inputs_cpu.py for
the preconditions those tests rely on): scatter, normalize, marginals and filter at the sizes at
which their kernels change path.  Plain functions, numpy only; nothing here touches the library
under test."""
import numpy

from tests._util import same_bits          # noqa: F401 -- the stage tests reach it through here

DBL_MAX = numpy.finfo(numpy.float64).max

# ---- normalize -----------------------------------------------------------------------------------
TILE, BIG_TILE, BIG_FROM = 32, 128, 256      # tile edges of the two kernels; the switch (d >= 256)

SWITCH_SIZES = [255, 256, 257]                 # 32-tile kernel | 128-tile kernel
SMALL_SIZES = [128, 129]                       # 32-tile kernel at a multiple of 128
TILE_EDGE_SIZES = [384, 385, 512, 513]         # 128-tile kernel: whole and ragged tiles
PERSISTENT_SIZES = [2816, 2817, 2945]          # 253 | 276 | 300 tile pairs: <= / > 256 CUs
THREE_TRIP_SIZE = 4225                         # 595 pairs = 2 x 256 + 83
NORMALIZE_SIZES = SMALL_SIZES + SWITCH_SIZES + TILE_EDGE_SIZES + PERSISTENT_SIZES


def tile_pairs(d, tile=BIG_TILE):
    """Tile pairs (TJ <= TK) of a (d, d) matrix: the work items of a normalize kernel."""
    nt = -(-int(d) // tile)
    return nt * (nt + 1) // 2


def trips(d, cus):
    """(most, fewest) trips a workgroup of normalize128_kernel makes at edge d when `cus`
    workgroups walk the pairs with stride `cus`."""
    p = tile_pairs(d)
    grid = min(p, cus)
    return -(-p // grid), p // grid


def has_three_trips(d, cus):
    """Some workgroup makes at least three trips at edge d and the last round is ragged (fewer
    pairs than workgroups)."""
    p = tile_pairs(d)
    return p > 2 * cus and p % cus != 0


def three_trip_size(cus):
    """An edge for which `has_three_trips` holds on a device of `cus` CUs: 4,225 (595 pairs)
    where it does -- 256 CUs among them -- else the smallest d = 128 k + 1 that does."""
    if has_three_trips(THREE_TRIP_SIZE, cus):
        return THREE_TRIP_SIZE
    nt = 1
    while not has_three_trips(nt * BIG_TILE, cus):
        nt += 1
    return (nt - 1) * BIG_TILE + 1


_SPECIALS = [0.0, -0.0, numpy.nan, numpy.inf, -numpy.inf, 5e-324, -5e-324, 1e-310, -2e-308]


def poison(d):
    """The value a strict-lower cell [r][c] of the dense map holds: 2^20 + (r d + c) + 1/2, finite
    and distinct per cell (exact in float64 up to d = 2^16)."""
    return 1048576.5 + numpy.arange(d * d, dtype=numpy.float64).reshape(d, d)


def dense_map(d):
    """The (d, d) input of the normalize tests, n_bins = d - 1.
      upper triangle and diagonal of the n_bins block: normal deviates times 2^-30 .. 2^30 (18
          orders of magnitude, both signs), a hundredth of the cells replaced by 0, -0.0, NaN,
          +-inf and denormals; the first nine diagonal cells hold those specials too;
      strict lower triangle of the block: `poison` -- unrelated to the mirrored upper cell, so a
          lower cell that was read, or left alone, shows;
      row n_bins and column n_bins: finite values, NaN and +-inf in patterns that differ between
          the two (the corner cell is -inf)."""
    n = d - 1
    rng = numpy.random.default_rng(1000 + d)
    m = rng.standard_normal((d, d))
    m = numpy.ldexp(m, rng.integers(-30, 31, size=(d, d), dtype=numpy.int32))
    cnt = max(9, d * d // 100)
    a, b = rng.integers(0, max(n, 1), cnt), rng.integers(0, max(n, 1), cnt)
    m[numpy.minimum(a, b), numpy.maximum(a, b)] = numpy.resize(_SPECIALS, cnt)
    k = min(n, len(_SPECIALS))
    m[numpy.arange(k), numpy.arange(k)] = _SPECIALS[:k]
    low = numpy.tri(d, d, -1, dtype=bool)
    low[n, :] = False
    m[low] = poison(d)[low]
    i = numpy.arange(d)
    row = (1.0 + i) * 0.375
    row[1::7], row[2::11], row[3::13] = numpy.nan, numpy.inf, -numpy.inf
    col = -(2.0 + i) * 1.75
    col[0::5], col[4::9], col[6::17] = numpy.nan, -numpy.inf, numpy.inf
    m[n, :] = row
    m[:, n] = col
    m[n, n] = -numpy.inf
    return m


def plain_kr(n_bins):
    """KRnorm in [0.5, 1.5) with a tenth NaN, KRexpected in [1, 2)."""
    rng = numpy.random.default_rng(2000 + n_bins)
    kr = 0.5 + rng.random(n_bins)
    kr[rng.random(n_bins) < 0.1] = numpy.nan
    return kr, 1.0 + rng.random(n_bins)


def extreme_kr(n_bins):
    """The plain vectors with extreme entries at fixed residues (KRnorm: index mod 32, KRexpected:
    distance mod 8), no exact zero among them.  For j = 3 (mod 32), k = j + 1 the divisor
    kr[j] * kr[k] * ke[1] is 1e200 * 1e200 * 1e-300: infinite left to right, 1e100 in any other
    association.  j = 6, k = 7: 1e-200 * 1e-200 underflows to 0 (x / 0, 0 / 0).  Also 1e+-300,
    negative, +-inf and denormal entries."""
    kr, ke = plain_kr(n_bins)
    i = numpy.arange(n_bins)
    for residue, value in ((3, 1e200), (4, 1e200), (6, 1e-200), (7, 1e-200), (9, 1e300),
                           (10, 1e-300), (13, numpy.inf), (14, -numpy.inf), (15, 5e-324)):
        kr[i % 32 == residue] = value
    neg = i % 32 == 12
    kr[neg] = -(1.0 + i[neg] / float(n_bins))
    for residue, value in ((1, 1e-300), (3, 1e300), (5, 1e-310), (7, -0.75)):
        ke[i % 8 == residue] = value
    return kr, ke


KR_FAMILIES = {"plain": plain_kr, "extreme": extreme_kr}


def pin_extreme_cells(m):
    """Numerators for the extreme vectors' fixed cells: [3][4] and [35][36] (infinite divisor)
    finite and not 0, [6][7] (zero divisor) not 0, [38][39] (zero divisor) 0."""
    m[3, 4], m[35, 36], m[6, 7], m[38, 39] = 3.0, -7.0, -5.0, 0.0
    return m


def divisor(kr, ke):
    """(n_bins, n_bins) array of (kr[j] * kr[k]) * ke[|k - j|], the product taken left to right."""
    n = kr.shape[0]
    i = numpy.arange(n)
    with numpy.errstate(all="ignore"):
        return (kr[:, None] * kr[None, :]) * ke[numpy.abs(i[None, :] - i[:, None])]


def normalize_numpy(m, kr, ke):
    """The reference's normalize loop stated in numpy, independent of the oracle: the upper
    triangle of the n_bins block divided by `divisor`, mirrored over the lower one, row and
    column n_bins untouched, then nan_to_num of the whole matrix.  Also returns the block's
    quotients before nan_to_num (their upper triangle is what the loop computes)."""
    n = m.shape[0] - 1
    with numpy.errstate(all="ignore"):
        quo = m[:n, :n] / divisor(kr[:n], ke[:n])
    upper = numpy.triu(numpy.ones((n, n), dtype=bool))
    out = numpy.array(m)
    out[:n, :n] = numpy.where(upper, quo, quo.T)      # bits copied, -0.0 included
    return numpy.nan_to_num(out), quo


# ---- marginals and filter ------------------------------------------------------------------------
FILTER_SIZES = [63, 64, 65, 128, 129, 255, 256, 257, 1023, 1024, 1025, 2048]


def ragged_map(d):
    """The recipe of test_contactmap_filter_vs_numpy_ragged: symmetric, values over 12 orders of
    magnitude (the order of a column's additions matters), a NaN and an inf column."""
    rng = numpy.random.default_rng(3000 + d)
    a = rng.standard_normal((d, d)) * 10.0 ** rng.integers(-6, 6, (d, d))
    m = a + a.T
    m[3, 5] = m[5, 3] = numpy.nan
    m[2, 7] = m[7, 2] = numpy.inf
    return m


def thresholds(marg):
    """(name, threshold) pairs: at a marginal, just above and just below it, at the median,
    nothing kept (+inf) and everything but the NaN column kept (-inf)."""
    fin = numpy.sort(marg[numpy.isfinite(marg)])
    at = float(fin[fin.size // 3])
    return [("at", at), ("above", float(numpy.nextafter(at, numpy.inf))),
            ("below", float(numpy.nextafter(at, -numpy.inf))),
            ("median", float(numpy.median(fin))), ("none", numpy.inf), ("all", -numpy.inf)]


def filter_numpy(m, thr):
    """(marginals, keep, filtered matrix) as numpy states them (datatypes.pyx:140-141).  The
    filtered matrix is returned C-contiguous, as the device holds it: `m[keep][:, keep]` itself
    is F-ordered, and numpy adds the columns of such an array in another order."""
    with numpy.errstate(all="ignore"):
        marg = m.sum(axis=0)
        keep = marg > thr
    return marg, keep, numpy.ascontiguousarray(m[keep][:, keep])


KEEP_EDGE = 2304       # edge of the keep-pattern maps: three 1,024-column chunks, the last ragged


def keep_patterns(d=KEEP_EDGE):
    """name -> boolean keep vector of length d.  keep_scan_kernel walks the columns in chunks of
    1,024 and carries the number kept so far; gather_kernel has 256 new columns per workgroup."""
    i = numpy.arange(d)
    rng = numpy.random.default_rng(d)
    scattered = numpy.zeros(d, dtype=bool)
    scattered[rng.choice(d, 512, replace=False)] = True
    dense256 = numpy.zeros(d, dtype=bool)
    dense256[900:1156] = True
    return {
        "first_kept_is_1024": i >= 1024,
        "first_kept_is_1023": i >= 1023,
        "last_kept_is_1023": i < 1024,
        "last_kept_is_1024": i <= 1024,
        "first_kept_is_2048": i >= 2048,
        "chunk0_empty_chunk1_full": (i >= 1024) & (i < 2048),
        "kept_512_scattered": scattered,
        "kept_256_across_a_chunk_edge": dense256,
        "kept_257": (i % 8 == 0) & (i < 8 * 257),
        "one_per_chunk": (i % 1024 == 1023) | (i == d - 1),
    }


def masked_map(keep):
    """Symmetric positive map whose bins outside `keep` have zero rows and columns, so that
    `filter(0)` keeps exactly `keep`."""
    d = keep.shape[0]
    m = numpy.random.default_rng(d + int(keep.sum())).random((d, d)) + 0.5
    m = numpy.triu(m) + numpy.triu(m, 1).T
    m[~keep, :] = 0.0
    m[:, ~keep] = 0.0
    return m


def pipeline_map(d):
    """Symmetric positive map whose marginals spread over three orders of magnitude (a scale per
    bin), for the filter -> marginals -> filter -> normalize -> marginals chain."""
    rng = numpy.random.default_rng(4000 + d)
    s = 10.0 ** (3.0 * rng.random(d))
    m = rng.random((d, d))
    m = numpy.triu(m) + numpy.triu(m, 1).T
    m *= s[:, None]
    m *= s[None, :]
    return m


def quantile_threshold(marg, kept):
    """A threshold that keeps exactly `kept` of the (distinct, finite) marginals."""
    s = numpy.sort(marg)
    assert numpy.unique(s).size == s.size and 0 < kept < s.size
    return float(s[s.size - kept - 1])


# ---- scatter -------------------------------------------------------------------------------------
def count_with_bits(bits):
    """The float64 whose bit pattern is the integer `bits`."""
    return float(numpy.array([bits], dtype=numpy.uint64).view(numpy.float64)[0])


def triples_of(bi, bj, counts, resolution, offset=0.0):
    """(n, 3) C-ordered rows [pos_i, pos_j, count], positions `offset` inside their bins."""
    return numpy.ascontiguousarray(numpy.stack(
        [numpy.asarray(bi) * float(resolution) + offset,
         numpy.asarray(bj) * float(resolution) + offset,
         numpy.asarray(counts, dtype=numpy.float64)], 1))


def layouts(rows):
    """(name, array) of the three memory layouts `ContactMap.from_triples` reads: C-ordered
    rows, the reference's F-ordered array, a strided view."""
    wide = numpy.zeros((rows.shape[0], 6))
    wide[:, ::2] = rows
    return [("C", rows), ("F", numpy.asfortranarray(rows)), ("strided", wide[:, ::2])]


def random_triples(n, n_bins, resolution, seed):
    """n triples over the bins 0 .. n_bins (the extra row included), about a tenth of them on the
    diagonal, distinct positive counts."""
    rng = numpy.random.default_rng(seed)
    bi = rng.integers(0, n_bins + 1, n)
    bj = rng.integers(0, n_bins + 1, n)
    diag = rng.random(n) < 0.1
    bj[diag] = bi[diag]
    return triples_of(bi, bj, 1.0 + numpy.arange(n) + rng.random(n), resolution)


def duplicate_triples(n_bins=300, resolution=5000, n=12000):
    """12,000 triples over the bins 0 .. 279 with many repeated cells, plus pinned repeats in
    the bins 280 .. 299, which the background leaves alone: (earlier index, later index,
    flipped) for each of one wave (3, 40), one workgroup (10, 200) and 10,000 apart
    (5, 10005), in one orientation and in both, and the same on diagonal cells.  Returns the
    rows and the list of pins (t1, t2, j, k)."""
    rng = numpy.random.default_rng(77)
    bi, bj = rng.integers(0, 280, n), rng.integers(0, 280, n)
    counts = 1.0 + numpy.arange(n) + rng.random(n)
    pins = []
    cell = 280
    for t1, t2 in ((3, 40), (10, 200), (5, 10005)):
        for kind in ("same", "flipped", "diagonal"):
            j, k = (cell, cell) if kind == "diagonal" else (cell, cell + 1)
            t1k, t2k = t1 + {"same": 0, "flipped": 11, "diagonal": 22}[kind], \
                t2 + {"same": 0, "flipped": 11, "diagonal": 22}[kind]
            bi[t1k], bj[t1k] = j, k
            bi[t2k], bj[t2k] = (k, j) if kind == "flipped" else (j, k)
            pins.append((t1k, t2k, j, k))
            cell += 2
    return triples_of(bi, bj, counts, resolution), pins


def mark_collision_triples(t2_of, n, n_bins=60, resolution=1000):
    """Triples in which a later triple's count has the bit pattern of an earlier triple's index
    + 1 (a float64 denormal) and both name the same cell:
      off-diagonal: t1 = 5 names (a, b), t2 = t2_of(5) names (b, a), bits(count[t2]) = 6;
      diagonal:     t1 = 20 names (e, e), t2 = t2_of(20) names (e, e), bits(count[t2]) = 21;
      and a later count that is a NaN whose payload is the earlier index + 1 (t1 = 30), which
      nan_to_num turns into 0.
    The other triples fill other cells.  Returns (rows, [(t1, t2, j, k)])."""
    rng = numpy.random.default_rng(n)
    bi, bj = rng.integers(0, 50, n), rng.integers(0, 50, n)
    counts = 1.0 + rng.random(n)
    pins = []
    for t1, (j, k), flip, nan in ((5, (52, 55), True, False), (20, (57, 57), False, False),
                                  (30, (53, 58), True, True)):
        t2 = t2_of(t1)
        bi[t1], bj[t1] = j, k
        bi[t2], bj[t2] = (k, j) if flip else (j, k)
        counts[t1] = 1000.0 + t1
        counts[t2] = count_with_bits((0xFFF8000000000000 if nan else 0) | (t1 + 1))
        pins.append((t1, t2, j, k))
    return triples_of(bi, bj, counts, resolution), pins
