"""The 24-bit stream of the fp32 stress sweep, restated in numpy from docs/SPEC.md 3.1-3.3 and 3.7
(never from the library): which units of a tile list a rank holds packed, the table of 3.7, the
wave chunks of 3.3, the strip changes a wave meets inside its chunk, and a float64 reference of
SPEC 2.3 / 2.4 / 2.4.1 over the stored cells of a tile list.  No GPU is needed here;
tests/test_pack24_model_cpu.py checks this file, tests/test_gpu_pack24.py and
tests/test_gpu_pack24_paths.py use it."""
import numpy

VW, RPU, UPT = 512, 4, 128          # fp32: 512-column strips, units of 4 rows, 128 units per tile
SPAN = 1 << 24
PACKED_KIB, RAW_KIB = 6, 8
WISH_FLOOR, F32_MAX = 1e-30, 3.4028234663852886e38
EPS2 = 1e-30                        # the floor under the square root of SPEC 2.2, fp32 runs


def uniform_map(n, seed=0, lo=1.0, hi=1.9):
    """Symmetric, zero diagonal, off-diagonal distances uniform in [lo, hi], exact in float32."""
    rng = numpy.random.default_rng(seed)
    w = rng.uniform(lo, hi, (n, n)).astype(numpy.float32).astype(numpy.float64)
    w = numpy.triu(w, 1)
    return w + w.T


def dense_tiles(n):
    """Tile list (I, J) of the dense upper triangle in device order: J ascending, then I."""
    nb = -(-int(n) // VW)
    I = [i for j in range(nb) for i in range(j + 1)]
    J = [j for j in range(nb) for i in range(j + 1)]
    return numpy.array(I, dtype=numpy.int32), numpy.array(J, dtype=numpy.int32)


def _tiles(n, tiles):
    I, J = dense_tiles(n) if tiles is None else tiles
    I, J = numpy.asarray(I, dtype=numpy.int64), numpy.asarray(J, dtype=numpy.int64)
    assert I.shape == J.shape and I.ndim == 1 and (I <= J).all()
    return I, J


def stored_tile(w, n, I, J):
    """The 512 x 512 stored words of tile (I, J) as float32: the wish distance of the cell where it
    is a constraint (finite, positive, inside [1e-30, the largest float32], SPEC 2.1), 0 on and
    below the diagonal and beyond bin n (SPEC 3.2)."""
    out = numpy.zeros((VW, VW), dtype=numpy.float32)
    r0, c0 = I * VW, J * VW
    r1, c1 = min(n, r0 + VW), min(n, c0 + VW)
    if r1 <= r0 or c1 <= c0:
        return out
    v = numpy.array(w[r0:r1, c0:c1], dtype=numpy.float64)
    with numpy.errstate(invalid="ignore"):
        keep = numpy.isfinite(v) & (v >= WISH_FLOOR) & (v <= F32_MAX)
    v = numpy.where(keep, v, 0.0)
    if I == J:
        v = numpy.triu(v, 1)
    out[:r1 - r0, :c1 - c0] = v.astype(numpy.float32)
    return out


def strip_of_unit(n, tiles=None, u_begin=0, u_end=None):
    """The column strip J of every unit of [u_begin, u_end) in storage order."""
    _, J = _tiles(n, tiles)
    strips = numpy.repeat(J, UPT)
    return strips[u_begin:strips.size if u_end is None else u_end]


def unit_spans(w, n, tiles=None):
    """(smallest, largest) stored word of every unit of the tile list, as uint32 in int64."""
    I, J = _tiles(n, tiles)
    lo = numpy.zeros(I.size * UPT, dtype=numpy.int64)
    hi = numpy.zeros(I.size * UPT, dtype=numpy.int64)
    for t in range(I.size):
        words = stored_tile(w, n, int(I[t]), int(J[t])).view(numpy.uint32).reshape(UPT, RPU * VW)
        lo[t * UPT:(t + 1) * UPT] = words.min(1)
        hi[t * UPT:(t + 1) * UPT] = words.max(1)
    return lo, hi


def run_rule(packable, min_run):
    """Stored packed: a packable unit inside a run of at least min_run consecutive packable units."""
    packable = numpy.asarray(packable, dtype=bool)
    packed = numpy.zeros(packable.shape, dtype=bool)
    a = 0
    while a < packable.size:
        b = a
        while b < packable.size and packable[b] == packable[a]:
            b += 1
        packed[a:b] = packable[a] and b - a >= min_run
        a = b
    return packed


def describe(packed, base):
    """(stream_info, table) of 3.7 from the per-unit packed mask and the units' smallest words.
    The table: `offset_kib`, where the unit begins in the stream (6 KiB per packed unit before it,
    8 per raw one), `packed`, and `base`, the unit's smallest word when packed and 0 otherwise.
    With no packed unit there is no stream: stream_bytes 0 (the table is still that of a stream
    of raw units)."""
    packed = numpy.asarray(packed, dtype=bool)
    size = numpy.where(packed, PACKED_KIB, RAW_KIB).astype(numpy.int64)
    offset = numpy.concatenate([[0], numpy.cumsum(size)[:-1]]) if packed.size else size
    table = {"offset_kib": offset, "packed": packed.copy(),
             "base": numpy.where(packed, numpy.asarray(base, dtype=numpy.int64), 0)}
    n_packed = int(packed.sum())
    if n_packed == 0:
        info = {"packed_units": 0, "raw_units": int(packed.size), "stream_bytes": 0, "format_switches": 0}
    else:
        info = {"packed_units": n_packed, "raw_units": int(packed.size) - n_packed,
                "stream_bytes": 1024 * int(size.sum()),
                "format_switches": int((packed[1:] != packed[:-1]).sum())}
    return info, table


def model(w, n, u_begin, u_end, min_run, tiles=None):
    """The rule, in numpy: the words of a unit are the float32 wish distances of its 4 rows x 512
    columns; packable: max - min < 2^24 as uint32; stored packed: inside a run of >= min_run
    packable units of the rank's order, units [u_begin, u_end) of the tile list (None: dense).
    Returns (stream_info, packed mask, table)."""
    lo, hi = unit_spans(w, n, tiles)
    lo, hi = lo[u_begin:u_end], hi[u_begin:u_end]
    packed = run_rule(hi - lo < SPAN, min_run)
    info, table = describe(packed, lo)
    return info, packed, table


def rank_range(n_units, rank, world):
    """SPEC 3.3: rank r of R owns the units [floor(U r / R), floor(U (r + 1) / R))."""
    return n_units * rank // world, n_units * (rank + 1) // world


# ---- the waves ----------------------------------------------------------------------------------
def waves_per_block(n_local, cus, waves_per_cu, pair=True):
    """fp32: workgroups of 8 waves with 8 or more waves per CU (and 8 or more waves), else of 4."""
    nw = max(1, min(cus * waves_per_cu, n_local))
    return 8 if pair and waves_per_cu >= 8 and nw >= 8 else 4


def chunks(n_local, cus, waves_per_cu, wpb):
    """The wave chunk rule: nw = round_up(max(1, min(cus * wpc, n_local)), wpb) waves, wave w owning
    the units [w q + min(w, r), + q (+ 1 if w < r)), q, r = divmod(n_local, nw).  A list of (a, b)."""
    nw = max(1, min(cus * waves_per_cu, n_local))
    nw = -(-nw // wpb) * wpb
    q, r = divmod(n_local, nw)
    out = []
    for w in range(nw):
        a = w * q + min(w, r)
        out.append((a, a + q + (1 if w < r else 0)))
    return out


def crossings(chunk_list, strips, packed):
    """The waves whose chunk holds a strip change -- units u - 1 and u of one chunk in different
    strips -- by the formats on its two sides: 'packed' (a: packed units on both sides),
    'packed_raw' and 'raw_packed' (b: a change of format at the change, in either direction), 'raw'
    (c: raw units on both sides).  Each a sorted list of wave numbers."""
    out = {"packed": set(), "packed_raw": set(), "raw_packed": set(), "raw": set()}
    name = {(True, True): "packed", (True, False): "packed_raw", (False, True): "raw_packed",
            (False, False): "raw"}
    for wv, (a, b) in enumerate(chunk_list):
        for u in range(a + 1, b):
            if strips[u] != strips[u - 1]:
                out[name[(bool(packed[u - 1]), bool(packed[u]))]].add(wv)
    return {k: sorted(v) for k, v in out.items()}


# ---- float64 reference over the stored cells --------------------------------------------------------
def stress_grad(w, n, X, tiles=None, u_begin=0, u_end=None):
    """SPEC 2.3 in float64 over the stored cells of units [u_begin, u_end) of the tile list: the
    wish distances are the float32 words (`stored_tile`), d = sqrt(|x_i - x_j|^2 + 1e-30).
    Returns (S, g) with g of shape (n, 3)."""
    I, J = _tiles(n, tiles)
    u_end = I.size * UPT if u_end is None else u_end
    X = numpy.asarray(X, dtype=numpy.float64)
    Xp = numpy.zeros((-(-n // VW) * VW, 3))
    Xp[:n] = X
    g = numpy.zeros_like(Xp)
    S = 0.0
    for t in range(u_begin // UPT, -(-u_end // UPT)):
        a, b = max(u_begin, t * UPT) - t * UPT, min(u_end, (t + 1) * UPT) - t * UPT
        if a >= b:
            continue
        delta = stored_tile(w, n, int(I[t]), int(J[t]))[a * RPU:b * RPU].astype(numpy.float64)
        r0, c0 = int(I[t]) * VW + a * RPU, int(J[t]) * VW
        xi, xj = Xp[r0:r0 + (b - a) * RPU], Xp[c0:c0 + VW]
        diff = xi[:, None, :] - xj[None, :, :]
        d = numpy.sqrt((diff * diff).sum(-1) + EPS2)
        on = delta > 0
        res = numpy.where(on, d - delta, 0.0)
        S += float((res * res).sum())
        f = (2.0 * res / d)[:, :, None] * diff
        g[r0:r0 + (b - a) * RPU] += f.sum(1)
        g[c0:c0 + VW] -= f.sum(0)
    return S, g[:n]


def run(w, n, x0, k, lr, mu=0.0, bin_scale=None, tiles=None):
    """K steps of SPEC 2.4 / 2.4.1 in float64: V <- mu V - lr c g, X <- X + V.  Returns
    (X_K, [S(X_0) .. S(X_{K-1})])."""
    X = numpy.array(x0, dtype=numpy.float64)
    V = numpy.zeros_like(X)
    c = None if bin_scale is None else numpy.asarray(bin_scale, dtype=numpy.float64)[:, None]
    hist = numpy.zeros(k)
    for it in range(k):
        hist[it], g = stress_grad(w, n, X, tiles)
        V = mu * V - lr * (g if c is None else c * g)
        X = X + V
    return X, hist


def map_tiles(tiles, bin_begin, m):
    """The tiles of a list that lie inside map m's bins [bin_begin[m], bin_begin[m + 1])."""
    I, J = numpy.asarray(tiles[0]), numpy.asarray(tiles[1])
    lo, hi = bin_begin[m] // VW, -(-bin_begin[m + 1] // VW)
    sel = (I >= lo) & (J < hi)
    return I[sel], J[sel]
