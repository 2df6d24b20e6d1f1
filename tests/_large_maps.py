"""Inputs and host references shared by the large-ContactMap tests
(tests/test_gpu_contactmap_large.py on the device, tests/test_contactmap_large_inputs_cpu.py for
the preconditions those tests rely on).  Plain functions, numpy only; nothing here touches the
library under test.

The matrices are those of the small-size tests in tests/test_gpu_parity.py -- the same formulas
and the same seeds (`default_rng(d)`), so that a size added here continues their series -- but
built without a d x d `**` (7 s at d = 8,193): the decay depends on |i - j| alone, so it is
raised to its power once per distance and laid out as a Toeplitz view."""
import numpy


def _toeplitz_view(first):
    """T[i, j] = first[|i - j|] as a read-only strided view (2 d doubles, no d x d array)."""
    d = first.shape[0]
    line = numpy.concatenate([first[:0:-1], first])            # line[d - 1 + k] = first[|k|]
    v = numpy.lib.stride_tricks.as_strided(line[d - 1:], shape=(d, d),
                                           strides=(-line.strides[0], line.strides[0]),
                                           writeable=False)
    return v


def _add_transpose(m, block=256):
    """m + m.T, in place and a block pair at a time through contiguous copies: a transposed
    walk over a matrix whose rows are a power of two apart (d = 8,192) lands in one cache set
    and takes several seconds.  m_ij + m_ji and m_ji + m_ij are the same float64."""
    d = m.shape[0]
    for i0 in range(0, d, block):
        for j0 in range(i0, d, block):
            a = m[i0:i0 + block, j0:j0 + block].copy()
            b = m[j0:j0 + block, i0:i0 + block].copy()
            m[i0:i0 + block, j0:j0 + block] = a + b.T
            if j0 > i0:
                m[j0:j0 + block, i0:i0 + block] = b + a.T
    return m


def _decaying(rng, d, scale, power):
    """rng.random((d, d)) * scale / (1 + |i - j|) ** power, symmetrised by adding the transpose:
    the bits of the d x d formula (asserted on the CPU at a small size)."""
    decay = (1.0 + numpy.arange(d)) ** power
    m = rng.random((d, d))
    m *= scale
    m /= _toeplitz_view(decay)
    return _add_transpose(m)


def hic_matrix(d):
    """The Hi-C-like map of test_contactmap_eigenvector_vs_scipy: positive, decaying as
    |i - j| ** -0.8."""
    return _decaying(numpy.random.default_rng(d), d, 50.0, 0.8)


def neg_matrix(d):
    """The indefinite map of the same test, whose eigenvalue of largest magnitude is negative
    (drawn from the generator after the Hi-C-like map's numbers, as there)."""
    rng = numpy.random.default_rng(d)
    rng.random((d, d))
    m = rng.standard_normal((d, d))
    m = m + m.T
    m -= 3.0 * numpy.sqrt(d) / max(d, 1)
    return m


def filter_eigen_map():
    """(matrix, dead bins) of the eigenvector-across-filter test: the Hi-C-like map of 4,200
    bins with the rows and columns of 200 of them zeroed, 4,000 left by `filter(0)`."""
    d = 4200
    m = hic_matrix(d)
    dead = numpy.sort(numpy.random.default_rng(7).choice(d, size=200, replace=False))
    m[dead, :] = 0.0
    m[:, dead] = 0.0
    return m, dead


EIGEN_FAMILIES = {"hic": hic_matrix, "neg": neg_matrix}


def corr_matrix(d):
    """The map of test_contactmap_correlation_vs_numpy: decaying as |i - j| ** -0.7."""
    return _decaying(numpy.random.default_rng(d), d, 40.0, 0.7)


def cheap_symmetric(d):
    """A symmetric float64 matrix of uniform [0, 1) entries for the sizes at which the decaying
    maps are too slow to make: ONE d x d array, drawn into in place, the upper triangle then
    copied over the lower one in cache-sized blocks (first touch of the array included: 4 s at
    d = 16,385, against 5 s for a float32 draw converted and symmetrised by adding)."""
    rng = numpy.random.default_rng(d)
    m = numpy.empty((d, d))
    rng.random(out=m.reshape(-1))
    b = 256
    for i0 in range(0, d, b):
        blk = m[i0:i0 + b, i0:i0 + b]
        blk[...] = numpy.triu(blk) + numpy.triu(blk, 1).T
        for j0 in range(i0 + b, d, b):
            m[j0:j0 + b, i0:i0 + b] = m[i0:i0 + b, j0:j0 + b].T
    return m


def integer_symmetric(d, rng, dead=None):
    """Symmetric, integer entries in [1, 2^20) as float64; rows and columns `dead` zeroed."""
    m = rng.integers(1, 1 << 20, size=(d, d)).astype(numpy.float64)
    m = numpy.triu(m) + numpy.triu(m, 1).T
    if dead is not None:
        m[dead, :] = 0.0
        m[:, dead] = 0.0
    return m


def integer_vector(d, rng):
    """Integers in [-1024, 1024] as float64."""
    return rng.integers(-1024, 1025, size=d).astype(numpy.float64)


def hic_like_counts(n, seed):
    """c_ij ~ Poisson(200 |i - j|^-1.08) with 2 % dead bins: the sparse maps of
    tests/test_gpu_shortest_paths.py."""
    r = numpy.random.default_rng(seed)
    i = numpy.arange(n)
    sep = numpy.abs(i[:, None] - i[None, :]).astype(numpy.float64)
    lam = 200.0 * numpy.maximum(sep, 1.0) ** -1.08
    numpy.fill_diagonal(lam, 0.0)
    c = numpy.triu(r.poisson(lam), 1).astype(numpy.float64)
    c += c.T
    dead = r.random(n) < 0.02
    c[dead, :] = 0.0
    c[:, dead] = 0.0
    return c


# ---- host references ---------------------------------------------------------------------------

def matvec_longdouble(m, v, slab=512):
    """m @ v in numpy.longdouble, the rows of `m` converted a slab at a time."""
    vl = numpy.asarray(v).astype(numpy.longdouble)
    out = numpy.empty(m.shape[0], dtype=numpy.longdouble)
    for lo in range(0, m.shape[0], slab):
        out[lo:lo + slab] = m[lo:lo + slab].astype(numpy.longdouble) @ vl
    return out


def residual_longdouble(m, theta, v):
    """(norm(m v - theta v), v^T m v) in numpy.longdouble, returned as floats."""
    vl = numpy.asarray(v).astype(numpy.longdouble)
    mv = matvec_longdouble(m, v)
    r = mv - numpy.longdouble(theta) * vl
    return float(numpy.sqrt(r @ r)), float(vl @ mv)


def fix_sign(u):
    """`u` with its component of largest magnitude made positive."""
    return u * numpy.sign(u[numpy.argmax(numpy.abs(u))])


def eigsh_largest(m, k=1):
    """scipy.sparse.linalg.eigsh(m, k) -- the reference project's own call -- sorted by
    decreasing magnitude: (eigenvalues, eigenvectors as columns)."""
    import scipy.sparse.linalg
    w, U = scipy.sparse.linalg.eigsh(m, k=k)
    order = numpy.argsort(-numpy.abs(w))
    return w[order], U[:, order]


def sample_rows(d, n_random=20):
    """The rows a sampled correlation reference looks at: both ends, the edges of the first
    64- and 128-row blocks and of the last 128-row block, the middle, and `n_random` more."""
    fixed = [0, 1, 63, 64, 127, 128, d // 2, d - 129, d - 128, d - 2, d - 1]
    more = numpy.random.default_rng(d + 1).integers(0, d, size=n_random).tolist()
    return numpy.array(sorted(set(r for r in fixed + more if 0 <= r < d)))


def corrcoef_rows(m, rows, in_place=False):
    """numpy.corrcoef(m)[rows] without the d x d product: rows centred, G = Xc[rows] @ Xc.T,
    divided by the row norms.  `in_place` centres `m` itself (no second matrix)."""
    xc = m if in_place else m.copy()
    xc -= xc.mean(axis=1, keepdims=True)
    norms = numpy.sqrt(numpy.einsum("ij,ij->i", xc, xc))
    g = xc[rows] @ xc.T
    with numpy.errstate(all="ignore"):
        g /= norms[rows][:, None]
        g /= norms[None, :]
    return g


def is_symmetric_bitwise(a, block=256):
    """a == a.T on the bit patterns (NaN equal to the same NaN), block by block."""
    bits = a.view(numpy.uint64)
    d = a.shape[0]
    for i0 in range(0, d, block):
        for j0 in range(i0, d, block):
            # (the lower block through a contiguous copy: see _add_transpose)
            if not numpy.array_equal(bits[i0:i0 + block, j0:j0 + block],
                                     bits[j0:j0 + block, i0:i0 + block].copy().T):
                return False
    return True
