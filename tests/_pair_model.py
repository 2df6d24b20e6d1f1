"""Test-only: a map whose bins have ONE partner each, and the solver's pair formula (docs/SPEC.md
2.2, 2.3, 2.3.1) per pair in numpy.longdouble.  Never imported by the package, and nothing of the
library is called here.

The matching.  The stored pairs (i, j), i < j, form a perfect matching: every other cell of the
wish matrix is 0 = no constraint, a masked pair adds +-0 to every sum, and the sums start at +0.0,
so g_i is what the pair arithmetic made of ONE pair, bit for bit, g_j its negation, and the stress
the plain sum of the pairs' res^2.  The matching is made of blocks of 2 o consecutive bins joined
at the offset o = j - i (bin b + t with bin b + t + o, t < o), o from OFFSETS: the small ones
cycle, and a large one follows every cycle while one takes no more than half of the bins left
(the largest: while it fits).
(The order of both lists was found by search, for 8 pairs or more at every position of every unit
layout -- 2 is the only offset that is 2 mod 4, so the fp32 unit needs many blocks of it;
tests/test_pair_model_cpu.py asserts what the matching reaches.)  With N odd the last bin has no
partner (the lonely bin).

The operands.  Pair p sits about its own midpoint, x_i = c + v, x_j = c - v, |c| <= |v|, with a
direction class (DIRECTIONS) and a ratio class delta / d (ratios(dtype)) assigned round-robin over
the pairs; one engine holds one scale 2^e, and d lies in [1/4, 5/8] 2^e.  Everything is rounded to
the run's dtype BEFORE the reference or the device sees it.

The reference.  d^2 = |x_i - x_j|^2 + eps^2 (eps^2 = the dtype's 1e-30 / 1e-300), d, res = d - delta,
coef = res / d * delta^-q, g_i = 2 coef (x_i - x_j), s = res^2 delta^-q, all in longdouble from the
dtype-rounded operands, and the terms the bounds are made of: 2 |x_i - x_j|_c (d + delta) / d *
delta^-q per component and (d + delta)^2 delta^-q per pair ((d + delta) for (d - delta): the
cancellation in res is then part of the bound, as in SPEC 4's score row)."""
import numpy

LD = numpy.longdouble
HAVE_LONGDOUBLE = numpy.finfo(LD).nmant >= 63
LONGDOUBLE_REASON = "numpy.longdouble has fewer than 64 significand bits here"

OFFSETS_SMALL = (5, 2, 3, 2, 1, 3, 2)          # one cycle of the small blocks
OFFSETS_LARGE = (1024 + 7, 65, 256, 64, 257, 255, 63, 511, 512, 513)
OFFSETS = tuple(sorted(set(OFFSETS_SMALL + OFFSETS_LARGE)))

# vw, rows per unit, columns per lane-load (16 bytes), as HipEngine.layout() reports the first two
LAYOUTS = {
    "f32": {"dtype": "float32", "vw": 512, "rows_per_unit": 4, "cols": 4},
    "f64n": {"dtype": "float64", "vw": 128, "rows_per_unit": 8, "cols": 2},
    "f64w": {"dtype": "float64", "vw": 512, "rows_per_unit": 2, "cols": 2},
}
SWEEP_SIZES = {"f32": 1537, "f64n": 1025, "f64w": 4097}
ROW_OWNER_SIZES = {"float32": (513,), "float64": (129, 1025)}
SCALES = {"float32": (-40, -12, 0, 12, 40), "float64": (-300, -40, 0, 40, 300)}
U = {"float32": LD(2) ** -24, "float64": LD(2) ** -53}
WISH_FLOOR = {"float32": 1e-30, "float64": 1e-290}

DIRECTIONS = ("x", "y", "z", "111", "122", "random")
EXACT = "delta = d"          # the ratio class that lives in direction "122" only
FLOOR = "wish floor"         # one pair of the e = 0 engine, q = 0


def np_dtype(dtype):
    return numpy.float32 if dtype == "float32" else numpy.float64


def eps2(dtype):
    """eps^2 of SPEC 2.2 as the kernels hold it: the dtype's rounding of 1e-30 / 1e-300."""
    return LD(numpy.float32(1e-30)) if dtype == "float32" else LD(1e-300)


def ratios(dtype):
    """delta / d of the ratio classes, as (name, value in longdouble)."""
    two = LD(2)
    out = [("2^-20", two ** -20), ("1/2", LD(0.5)), ("1-2^-10", 1 - two ** -10),
           ("1-2^-20", 1 - two ** -20), ("1+2^-20", 1 + two ** -20), ("2", two), ("2^20", two ** 20)]
    if dtype == "float64":
        out += [("1-2^-40", 1 - two ** -40), ("1+2^-40", 1 + two ** -40)]
    return out


# ---- the matching -----------------------------------------------------------------------------
def matching(n):
    """(i, j, offset) of the n // 2 pairs, in bin order of i within each block, and the lonely
    bins (none, or the last)."""
    pi, pj, po = [], [], []
    pos = 0
    large = list(OFFSETS_LARGE)

    def block(o):
        nonlocal pos
        t = numpy.arange(o)
        pi.append(pos + t)
        pj.append(pos + t + o)
        po.append(numpy.full(o, o))
        pos += 2 * o

    while n - pos >= 2:
        for o in OFFSETS_SMALL:
            if n - pos >= 2 * o:
                block(o)
        while large and n - pos < (2 if large[0] == max(OFFSETS_LARGE) else 4) * large[0]:
            large.pop(0)
        if large:
            block(large.pop(0))
    i, j, o = (numpy.concatenate(a).astype(numpy.int64) for a in (pi, pj, po))
    return i, j, o, list(range(pos, n))


def positions(layout, i, j):
    """Where pair (i, j) sits in the unit sweep of `layout`: the template arguments of the pair
    steps.  row: matrix row within the unit (R); load: which of a lane's loads of the row (K);
    col: column within the load (H and the half of a packed pair, or C); lane; and whether the
    tile is a diagonal one."""
    lay = LAYOUTS[layout]
    vw, cols = lay["vw"], lay["cols"]
    per_load = 64 * cols
    return {"row": i % lay["rows_per_unit"], "load": (j % vw) // per_load, "col": j % cols,
            "lane": (j % per_load) // cols, "diag": (i // vw) == (j // vw)}


def position_class(layout, i, j):
    """One integer per combination of (row, load, col) and the number of combinations."""
    lay = LAYOUTS[layout]
    p = positions(layout, i, j)
    loads = lay["vw"] // (64 * lay["cols"])
    return (p["row"] * loads + p["load"]) * lay["cols"] + p["col"], lay["rows_per_unit"] * loads * lay["cols"]


def row_owner_class(dtype, i, j):
    """The row owner: which of a lane's columns of a trip the partner is, from either end."""
    cols = 4 if dtype == "float32" else 2
    return j % cols, i % cols, cols


# ---- the operands -----------------------------------------------------------------------------
class Case(object):
    """One engine's input: x (n, 3) and delta per pair as float64 holding dtype values."""


def operands(n, dtype, e, q=0, layout=None, seed=0):
    """The pairs, coordinates and wish distances of the engine of scale 2^e.  The classes go
    round-robin over the pairs of each position class (of the unit sweep of `layout`; None: of
    the row owner): the k-th pair of a position takes ratio k mod R and direction (k + k div R)
    mod 6, so that R pairs of a position meet every ratio and every direction.  Past the first
    round the "122" pairs of the second take delta = d, and the first pair past it, in the
    e = 0 engine at q = 0, delta at the wish floor."""
    T = np_dtype(dtype)
    i, j, off, lonely = matching(n)
    m = i.size
    rng = numpy.random.default_rng(1000 * seed + n)
    rat = ratios(dtype)
    R = len(rat)
    if layout is None:
        at_j, at_i, cols = row_owner_class(dtype, i, j)
        cls = at_j * cols + at_i
    else:
        cls, _ = position_class(layout, i, j)
    rank = numpy.zeros(m, dtype=numpy.int64)
    for c in numpy.unique(cls):
        k = numpy.flatnonzero(cls == c)
        rank[k] = numpy.arange(k.size)
    rcls = rank % R
    dcls = (rank + rank // R) % len(DIRECTIONS)
    exact = (dcls == DIRECTIONS.index("122")) & (rank >= R) & (rank < 2 * R)
    past = numpy.flatnonzero((rank >= R) & ~exact)
    scale = LD(2) ** e
    mant = 1.0 + rng.integers(0, 8, m) / 16.0                  # 1 .. 1.4375, 4 bits
    x = numpy.zeros((n, 3))
    # structured directions: x_i - x_j = 2 dir h, the midpoint on the grid h / 4 -- all exact
    dirs = {"x": ((1, 0, 0), 3.0 / 16), "y": ((0, 1, 0), 3.0 / 16), "z": ((0, 0, 1), 3.0 / 16),
            "111": ((1, 1, 1), 1.0 / 8), "122": ((1, 2, 2), 1.0 / 16)}
    v = numpy.zeros((m, 3), dtype=LD)
    c = numpy.zeros((m, 3), dtype=LD)
    sign = rng.choice([-1.0, 1.0], (m, 3))
    for name, (d3, h0) in dirs.items():
        k = dcls == DIRECTIONS.index(name)
        h = (mant[k] * h0).astype(LD) * scale
        v[k] = numpy.asarray(d3, dtype=LD)[None, :] * sign[k] * h[:, None]
        c[k] = rng.integers(-2, 3, (int(k.sum()), 3)) * (h[:, None] / 4)
    k = dcls == DIRECTIONS.index("random")
    r = rng.uniform(0.5, 1.0, (int(k.sum()), 3)) * sign[k]
    r *= (rng.uniform(0.25, 0.625, int(k.sum())) / 2 / numpy.sqrt((r * r).sum(1)))[:, None]
    v[k] = r.astype(LD) * scale
    c[k] = (rng.uniform(-0.5, 0.5, (int(k.sum()), 3)) * numpy.abs(r)).astype(LD) * scale
    x[i] = (c + v).astype(T).astype(numpy.float64)
    x[j] = (c - v).astype(T).astype(numpy.float64)
    for b in lonely:
        x[b] = (numpy.asarray([0.3, -0.2, 0.1], dtype=LD) * scale).astype(T).astype(numpy.float64)
    d = pair_distance(x, i, j, dtype)
    ratio = numpy.asarray([rat[a][1] for a in rcls], dtype=LD)
    delta = numpy.where(exact, d, ratio * d).astype(T).astype(numpy.float64)
    names = [EXACT if exact[a] else rat[rcls[a]][0] for a in range(m)]
    if e == 0 and q == 0:
        floor = T(WISH_FLOOR[dtype])
        if float(floor) < WISH_FLOOR[dtype]:
            floor = numpy.nextafter(floor, T(1))
        delta[past[0]], names[past[0]] = float(floor), FLOOR
    out = Case()
    out.n, out.dtype, out.e, out.q = n, dtype, e, q
    out.i, out.j, out.offset, out.lonely = i, j, off, lonely
    out.x, out.delta = x, delta
    out.direction = [DIRECTIONS[a] for a in dcls]
    out.ratio = names
    return out


# ---- the reference ----------------------------------------------------------------------------
def pair_distance(x, i, j, dtype):
    dx = x[i].astype(LD) - x[j].astype(LD)
    return numpy.sqrt((dx * dx).sum(1) + eps2(dtype))


class Reference(object):
    """Per pair p: g (m, 3) = the gradient of bin i (bin j: its negation), s (m,) = the pair's
    stress term, unit_g (m, 3) and unit_s (m,) = what the bounds multiply C u and (n + C_S) u by."""


def reference(case, q):
    x, i, j = case.x, case.i, case.j
    delta = case.delta.astype(LD)
    dx = x[i].astype(LD) - x[j].astype(LD)
    d = numpy.sqrt((dx * dx).sum(1) + eps2(case.dtype))
    res = d - delta
    w = delta ** (-q) if q else numpy.ones_like(delta)
    out = Reference()
    out.d, out.res = d, res
    out.g = (2 * res / d * w)[:, None] * dx
    out.s = res * res * w
    out.unit_g = (2 * (d + delta) / d * w)[:, None] * numpy.abs(dx)
    out.unit_s = (d + delta) ** 2 * w
    return out


def wish_triples(case):
    """rows, cols, vals of the matching for set_wish_sparse (each pair once, i < j)."""
    return case.i, case.j, case.delta


# ---- the counted roundings ----------------------------------------------------------------------
# Per copy and weight power: how many roundings of size u = 2^-24 / 2^-53 the code, read as it
# stands, can put between the exact g_i (stress term) of the dtype-rounded operands and its own,
# in units of the bound terms above, every one taken in the same direction.  The tests assert at
# C = 2 * count.  How each figure is counted: docs/MEASUREMENTS.md, "the pair arithmetic".
#   dx                   1    (one subtract)
#   d2                   2 dx + the roundings of the longest chain: fma form 3, mul + add form 4
#   rsq / rcp (fp32)     1 ulp = 2; rsqrt_sqrt_f64, rcp_f64: 2 ulp = 4
#   rinv                 d2 / 2 + the routine
#   dist                 fp32: d2 / 2 + rsq + the product d2 * rinv; fp64: d2 / 2 + the routine
#   res                  dist + 1, from here on in units of u (d + delta)
#   coef, g              one per product, plus the factors' own
COUNTS = {
    # copy: {q: (gradient count, stress count)}
    "f32 sweep": {0: (15, 17), 1: (18, 20), 2: (19, 21)},
    "f32 row owner": {0: (14, 14), 1: (17, 17), 2: (20, 20)},
    "f64 sweep": {0: (17, 16), 1: (22, 21), 2: (27, 26)},
    "f64 row owner": {0: (17, 16), 1: (22, 21), 2: (27, 26)},
}


def bound_factors(copy, q):
    """(C, C_S): twice the counts."""
    g, s = COUNTS[copy][q]
    return 2 * g, 2 * s
