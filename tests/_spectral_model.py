"""The spectral start written from its definition in numpy float64, the maps the
spectral tests run on, and the list of cases the GPU file and the CPU precondition file share.
No library code: nothing here imports blueberry_amd, so what tests/test_gpu_spectral.py compares
the device with is independent of the device and of solver.py's host-driven loop."""
import collections
import functools

import numpy

# the sweep tolerances of BASELINE.json (fp64 1e-12, fp32 1e-5): what a product may be off by
TOL_T = {"float64": 1e-12, "float32": 1e-5}
# the bounds of test_spectral_init_recovers_exact_distances on a complete noise-free map
TOL_EXACT = {"float64": 1e-9, "float32": 1e-3}


# ---- the packers' rule and the product ------------------------------------------------------
def clean_wish(m, kind="wish", alpha=3.0):
    """What the packers make of an input matrix (`wish_from_value`): only the upper triangle is
    read; a value that is finite and positive is kept (counts: v ** (-1 / alpha)), everything
    else is 0 = no constraint; zero diagonal, symmetric.  (SPEC 2.1 also drops a distance below
    the wish floor or above the largest finite value of the solver's dtype -- 1e-30 and 3.4e38
    in fp32: tests/_input_model.wish_from_value has the rule per dtype; no map of the spectral
    tests comes near either.)"""
    u = numpy.triu(numpy.asarray(m, dtype=numpy.float64), 1)
    ok = numpy.isfinite(u) & (u > 0.0)
    v = numpy.zeros_like(u)
    v[ok] = u[ok] ** (-1.0 / alpha) if kind == "counts" else u[ok]
    return v + v.T


def matvec_sq_ref(w, x):
    """(w o w) @ x in float64."""
    w = numpy.asarray(w, dtype=numpy.float64)
    return (w * w) @ numpy.asarray(x, dtype=numpy.float64)


def matvec_sq_int(w, x):
    """The same for integer w and x, in int64: exact."""
    wi, xi = numpy.asarray(w).astype(numpy.int64), numpy.asarray(x).astype(numpy.int64)
    assert numpy.array_equal(wi, w) and numpy.array_equal(xi, x)
    return (wi * wi) @ xi


def matvec_sq_int_entries(n, rows, cols, vals, x):
    """The int64 product of a map given as entries (each pair once, i != j)."""
    r, c = numpy.asarray(rows, dtype=numpy.int64), numpy.asarray(cols, dtype=numpy.int64)
    v, xi = numpy.asarray(vals).astype(numpy.int64), numpy.asarray(x).astype(numpy.int64)
    assert numpy.array_equal(v, vals) and numpy.array_equal(xi, x) and (r != c).all()
    y = numpy.zeros((n, 3), dtype=numpy.int64)
    a = (v * v)[:, None]
    numpy.add.at(y, r, a * xi[c])
    numpy.add.at(y, c, a * xi[r])
    return y


# ---- the iteration ---------------------------------------------------------------------------
Start = collections.namedtuple("Start", "x0 products residuals ritz")


def spectral_ref(op, v0, k, tol=0.0, perturb=0.0, seed=0):
    """Classical MDS by block power iteration, from the definition.  op(U) = (D o D) U for an
    (n, 3) array U; B V = -1/2 J op(J V), J = I - 11'/n.  V = qr(v0); at most k times:
    Z = B V, [leave if tol > 0, this is not the first product and the distance of Z from
    span(V), sqrt(max(0, |Z|^2 - |V'Z|^2) / |Z|^2), is below tol], V = qr(Z).  Then the
    Rayleigh-Ritz step on sym(V'Z) with the last product (one more if the loop ran out), every
    Ritz vector turned to the side of v0[:, 0], X0 = U sqrt(max(lambda, 0)).

    Returns (x0, products, residuals, ritz): `products` counts the products that were
    orthonormalised (what bb_solver_spectral_init_tol reports: the Rayleigh-Ritz step's own
    product is not among them), `residuals` has the distance of EVERY product made, the
    Rayleigh-Ritz step's included, `ritz` the three Ritz values in descending order.

    perturb = p: every product is multiplied element-wise by 1 + p xi, xi uniform in [-1, 1]
    from `seed` -- how far the start moves when each product is off by p."""
    v0 = numpy.asarray(v0, dtype=numpy.float64)
    n = v0.shape[0]
    rng = numpy.random.default_rng(seed)

    def apply_B(V):
        W = numpy.asarray(op(V - V.mean(axis=0)), dtype=numpy.float64)
        if perturb:
            W = W * (1.0 + perturb * rng.uniform(-1.0, 1.0, W.shape))
        return -0.5 * (W - W.mean(axis=0))

    def orth(A):
        Q = numpy.linalg.qr(A)[0]
        if Q.shape[1] < 3:                       # fewer than 3 bins
            Q = numpy.hstack([Q, numpy.zeros((n, 3 - Q.shape[1]))])
        return Q

    def distance(V, Z):
        zz, G = float((Z * Z).sum()), V.T @ Z
        return numpy.sqrt(max(0.0, zz - float((G * G).sum())) / zz) if zz > 0.0 else 0.0

    V, Z, done, residuals = orth(v0), None, 0, []
    for it in range(int(k)):
        Z = apply_B(V)
        residuals.append(distance(V, Z))
        if tol > 0.0 and it > 0 and residuals[-1] < tol:
            break
        V, Z = orth(Z), None
        done = it + 1
    if Z is None:
        Z = apply_B(V)
        residuals.append(distance(V, Z))
    G = V.T @ Z
    lam, E = numpy.linalg.eigh(0.5 * (G + G.T))
    order = numpy.argsort(lam)[::-1]
    U = V @ E[:, order]
    U = U * numpy.where(U.T @ v0[:, 0] < 0.0, -1.0, 1.0)
    return Start(U * numpy.sqrt(numpy.maximum(lam[order], 0.0)), done, residuals, lam[order])


def dense_op(w):
    a = numpy.asarray(w, dtype=numpy.float64) ** 2
    return lambda U: a @ U


def complete_op(xs):
    """(D o D) U of the complete noise-free map of the coordinates xs, D_ij = |x_i - x_j|, in
    O(n): |x_i|^2 sum(U) - 2 x_i (sum_j x_j U_j') + sum_j |x_j|^2 U_j."""
    xs = numpy.asarray(xs, dtype=numpy.float64)
    r2 = (xs * xs).sum(axis=1)
    return lambda U: r2[:, None] * U.sum(axis=0)[None, :] - 2.0 * (xs @ (xs.T @ U)) + (r2 @ U)[None, :]


def movement(op, v0, k, tol, dtype, ref=None):
    """m: how far (relative to max |X0|) the model's start moves when every product is off by
    the sweep tolerance of `dtype`.  One draw of the perturbation."""
    ref = spectral_ref(op, v0, k, tol) if ref is None else ref
    moved = spectral_ref(op, v0, k, tol, perturb=TOL_T[dtype], seed=1)
    return float(numpy.abs(moved.x0 - ref.x0).max() / numpy.abs(ref.x0).max()), moved


# ---- maps -------------------------------------------------------------------------------------
def random_walk(n, seed=0):
    """tests/_oracle.random_walk: a 3-D Gaussian random walk, centred."""
    x = numpy.cumsum(numpy.random.default_rng(seed).standard_normal((n, 3)), axis=0)
    return x - x.mean(axis=0)


def pair_distances(x, block=512):
    """|x_i - x_j| for all pairs, made in blocks of rows (no (n, n, 3) array)."""
    x = numpy.asarray(x, dtype=numpy.float64)
    out = numpy.empty((x.shape[0], x.shape[0]))
    for a in range(0, x.shape[0], block):
        d = x[a:a + block, None, :] - x[None, :, :]
        out[a:a + block] = numpy.sqrt((d * d).sum(-1))
    return out


def start_block(n, seed=0):
    """The v0 StructureSolver(seed=seed) hands to the spectral start."""
    return numpy.random.default_rng(seed).standard_normal((n, 3))


@functools.lru_cache(maxsize=8)
def walk_map(n, seed=0):
    """(xs, w): the complete noise-free map of random_walk(n, seed)."""
    xs = random_walk(n, seed)
    w = pair_distances(xs)
    w.setflags(write=False)
    return xs, w


@functools.lru_cache(maxsize=32)
def holed_map(n, seed=0, fraction=0.1):
    """walk_map with `fraction` of its pairs removed, symmetrically."""
    w = walk_map(n, seed)[1].copy()
    hole = numpy.triu(numpy.random.default_rng(seed + 5).random((n, n)) < fraction, 1)
    w[hole | hole.T] = 0.0
    w.setflags(write=False)
    return w


def band_entries(n, half_width, seed=0):
    """(rows, cols, vals) of a band map with small-integer wish distances: every pair
    0 < j - i <= half_width once, in the upper triangle, values in {0, 1, 2, 3} (0 = no
    constraint, about a quarter of them)."""
    rng = numpy.random.default_rng(seed)
    i = numpy.repeat(numpy.arange(n, dtype=numpy.int64), half_width)
    j = i + numpy.tile(numpy.arange(1, half_width + 1, dtype=numpy.int64), n)
    keep = j < n
    i, j = i[keep], j[keep]
    return i, j, rng.integers(0, 4, i.size).astype(numpy.float64)


def integer_map(n, seed=0):
    """A dense symmetric map with wish distances in {0, 1, 2, 3}, about a quarter zeros."""
    u = numpy.triu(numpy.random.default_rng(seed).integers(0, 4, (n, n)), 1).astype(numpy.float64)
    return u + u.T


def integer_rhs(n, seed=0):
    """Three right-hand sides with integer entries in [-2, 2]."""
    return numpy.random.default_rng(seed + 1000).integers(-2, 3, (n, 3)).astype(numpy.float64)


def with_junk(w, seed=0):
    """`w` as an input the packers have to clean: a non-zero diagonal, NaN / +inf / -inf /
    negative values in a tenth of the pairs, and nothing but junk below the diagonal.
    clean_wish(result) is the map the device should hold."""
    n = w.shape[0]
    rng = numpy.random.default_rng(seed + 77)
    junk = numpy.array([numpy.nan, numpy.inf, -numpy.inf, -1.0, -3.0])
    m = numpy.triu(numpy.asarray(w, dtype=numpy.float64), 1)
    hit = numpy.triu(rng.random((n, n)) < 0.1, 1)
    m[hit] = junk[rng.integers(0, junk.size, int(hit.sum()))]
    low = numpy.tril(numpy.ones((n, n), dtype=bool), -1)
    m[low] = junk[rng.integers(0, junk.size, int(low.sum()))]
    m[numpy.arange(n), numpy.arange(n)] = rng.integers(1, 4, n)
    return m


MAX_EXACT = 2 ** 24          # every integer up to here is a float32


def largest_partial_sum(w, x):
    """max_i sum_j w_ij^2 |x_j|: no partial sum of the product, in any order, exceeds it."""
    return float(((numpy.asarray(w) ** 2) @ numpy.abs(x)).max())


# ---- maps without three directions (3e) -----------------------------------------------------
DEGENERATE = ("line", "plane", "three_points", "empty", "single_edge")


def degenerate_map(kind, n, seed=0):
    """(w, exact): a map whose B has rank below 3.  `exact` says that w is a complete
    noise-free Euclidean map (classical MDS reproduces its distances): points on a line, on a
    plane, at three generic places (bin i sits at place i % 3; coincident bins have distance
    0, which is also what "no constraint" embeds as).  The empty map and the map whose only
    pair is (0, 1) are not."""
    rng = numpy.random.default_rng(seed + 11 * n)
    if kind == "empty":
        return numpy.zeros((n, n)), False
    if kind == "single_edge":
        w = numpy.zeros((n, n))
        w[0, 1] = w[1, 0] = 2.5
        return w, False
    if kind == "line":
        xs = numpy.outer(numpy.cumsum(rng.random(n) + 0.5), [0.6, -0.5, 0.3])
    elif kind == "plane":
        xs = numpy.cumsum(rng.standard_normal((n, 2)), axis=0) @ numpy.array([[1.0, 0.2, -0.3],
                                                                               [0.1, 0.9, 0.5]])
    elif kind == "three_points":
        xs = (rng.standard_normal((3, 3)) * 3.0)[numpy.arange(n) % 3]
    else:
        raise ValueError(kind)
    return pair_distances(xs), True


# ---- the cases of tests/test_gpu_spectral.py, shared with their precondition tests -----------
SIZES_MATVEC = (2, 3, 7, 8, 9, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1025, 4096, 4097)
SIZES_PRODUCTS = (4, 5, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025)
K_PRODUCTS = (0, 1, 3)
STOP_CASES = tuple((n, tol) for n in (257, 1025) for tol in (1e-2, 1e-3))
STOP_CAP = 80
DTYPES = ("float64", "float32")


# The generators' seeds.  A case has to meet the preconditions tests/test_spectral_model_cpu.py
# asserts (Ritz values apart from 0 and from one another, no residual within a factor 2 of the
# stopping tolerance); the seed is n unless that map misses one of them, then the next that
# meets them all (of the 14 k-products sizes only 1,024 needed another seed).  The residuals of
# these maps fall by a factor of 1.1 to 4 per product, so a stopping case needs a map whose
# residual happens to jump over [tol / 2, 2 tol], and few do: these four are hand-picked, not
# typical.  Seeds tried from 0 upwards, and those that met everything: n = 257, tol = 1e-2:
# 3,000 tried, 2 met (2469, 2705); n = 257, tol = 1e-3: 120 tried, 1 met (51); n = 1,025,
# tol = 1e-2: 298 tried, 3 met (142, 230, 297); n = 1,025, tol = 1e-3: 120 tried, 2 met (44, 59).
_PRODUCTS_SEED = {1024: 1025}
_STOP_SEED = {(257, 1e-2): 2469, (257, 1e-3): 51, (1025, 1e-2): 142, (1025, 1e-3): 44}


def products_case(n):
    """(w, v0) of the k-products cases: a random walk with 10 % of its pairs removed."""
    seed = _PRODUCTS_SEED.get(n, n)
    return holed_map(n, seed=seed), start_block(n, seed=seed)


def stop_case(n, tol):
    seed = _STOP_SEED[(n, tol)]
    return holed_map(n, seed=seed), start_block(n, seed=seed)


ILL_N, ILL_C = 300, 1e6


def ill_conditioned_case():
    """(w, v0, g): the k-products map of ILL_N bins with a start block whose columns are nearly
    parallel, v0 = [g0, g0 + g1 / c, g0 + g2 / c] with c = ILL_C (cond(v0) about c), g the
    well-conditioned block it is made from.  span(v0) = span(g) and the sign rule reads g0 in
    both, so the start of v0 is the start of g; but the library orthonormalises v0 by two passes
    of Cholesky-QR, and one pass alone leaves cond(v0)^2 eps of it unorthogonal."""
    w, g = products_case(ILL_N)
    v0 = numpy.column_stack([g[:, 0], g[:, 0] + g[:, 1] / ILL_C, g[:, 0] + g[:, 2] / ILL_C])
    return w, v0, g
