"""ContactMap -- the solver's input datatype.

Mirrors the public surface of the reference's Cython class
(`blueberry/datatypes.pyx:31-272`): same constructor arguments, public
attributes (pyx:78-86), in-place / return-None methods and the
`(n_bins+1, n_bins+1)` float64 matrix.  The two Cython loops of the class --
the sparse-triple scatter (pyx:110-116) and KR + observed/expected
normalisation (pyx:166-169, nan_to_num :171) -- run on the GPU through
libblueberry_hip.so and are bit-exact against golden vectors captured from
the real reference (tests/golden/contactmap.npz).  Everything the reference
does with numpy / scipy / pandas stays numpy / scipy / pandas here.

Deviations from the reference, all deliberate:
  * `from_arrays` works: the reference's calls the file-loading constructor
    and has no `return` (pyx:264-272), so it needs the lab's NFS files and
    yields None.  Here it builds the map from the arrays alone, and takes
    optional KRnorm / KRexpected so that `normalize()` is usable.
  * path templates use `resolution // 1000` (the Python 2 meaning of the
    reference's `resolution/1000`, pyx:90-95).
  * `filter` also updates `n_bins` (= rows kept) and `regions` (the reference
    leaves them stale, pyx:140-141) and drops the KR vectors, so a later
    `normalize()` raises instead of indexing out of bounds --
    `keep_stale=True` restores the old behaviour.  The matrix it leaves is bit
    for bit the reference's (goldens `cm*_filter_*`).
  * `matrix` is a lazily fetched attribute, read-only while the matrix lives in HBM
    (class docstring); `to_host()`, `host_matrix()`, `marginals()`, `from_triples()`
    are additions.
  * `normalize` raises ZeroDivisionError up front when a divisor would be 0
    (the reference raises from inside the loop, after modifying part of the
    matrix, because Cython checks float division; golden flag
    `cm_zero_kr_raises_zerodivision`).
"""
import numpy

from . import _lib
from .ranks import pick_device, several_ranks
from .resolution import check_factor
from .utils import Q_LOWER_BOUND

RAO ="/net/noble/vol1/data/hic-datasets/"
RAW_DIR = RAO + ("data/Rao-Cell2014/rawFromGEO/{0}/{2}kb_resolution_intrachromosomal/chr{1}/"
                 "MAPQGE30/chr{1}_{2}kb.RAWobserved")
KR_NORM = RAO + ("data/Rao-Cell2014/rawFromGEO/{0}/{2}kb_resolution_intrachromosomal/chr{1}/"
                 "MAPQGE30/chr{1}_{2}kb.KRnorm")
KR_EXP = RAO + ("data/Rao-Cell2014/rawFromGEO/{0}/{2}kb_resolution_intrachromosomal/chr{1}/"
                "MAPQGE30/chr{1}_{2}kb.KRexpected")


def scatter_triples(triples, resolution, n_bins, device=0):
    """(n,3) [pos_i, pos_j, count] rows -> dense symmetric (n_bins+1)^2 host matrix.

    GPU form of the loop at `blueberry/datatypes.pyx:110-116`: bin =
    int(pos / resolution), both [j,k] and [k,j] set, later rows win."""
    return _DeviceMatrix.from_triples(triples, resolution, n_bins, device).to_host()


def _assign_last_wins(matrix, rows, cols, vals):
    """matrix[rows[k], cols[k]] = vals[k] for k in order -- of several entries for one cell
    the LAST stays, as in the reference's Python loops (`blueberry/datatypes.pyx:268-271,
    376-386`) -- without a Python loop over the entries: numpy leaves the outcome of a fancy
    assignment with repeated indices open, so the last entry of every cell is picked first."""
    if rows.shape[0] == 0:
        return
    flat = rows.astype(numpy.int64) * matrix.shape[1] + cols.astype(numpy.int64)
    # unique() on the reversed keys returns, per cell, its first index there = its last here
    _, first_rev = numpy.unique(flat[::-1], return_index=True)
    last = flat.shape[0] - 1 - first_rev
    matrix.reshape(-1)[flat[last]] = numpy.asarray(vals)[last]


def _nan_to_num(a):
    """`numpy.nan_to_num` of a float64 view of `a` (pyx:102) -- without the copy and the
    three passes when every value is finite already (10 M triples: 36 ms instead of 0.7 s).
    Host paths only: the device scatter applies nan_to_num to the values as it reads them."""
    a = numpy.asarray(a, dtype=numpy.float64)
    return a if numpy.isfinite(a).all() else numpy.nan_to_num(a)


def triples_buffer(triples):
    """(t, buf, row_major) of a `triples` argument: t, its float64 (n, 3) view (ValueError for
    another shape); buf, the array C reads, and whether it holds t row by row.  C-ordered rows
    are read in place; the reference's own layout -- pandas hands it an F-ordered array and its
    pointer arithmetic reads that column-major (pyx:111-113) -- is read in place too; anything
    else is copied once."""
    t = numpy.asarray(triples, dtype=numpy.float64)
    if t.ndim != 2 or t.shape[1] != 3:
        raise ValueError("triples must have shape (n, 3)")
    if t.flags.c_contiguous:
        return t, t, 1
    if t.flags.f_contiguous:
        return t, t.T, 0
    return t, numpy.ascontiguousarray(t), 1


class _DeviceMatrix(_lib.Handle):
    """Owner of one bb_cm handle: the (d, d) float64 matrix resident in HBM."""
    prefix = "bb_cm_"

    def __init__(self, d, device):
        _lib.Handle.__init__(self)
        self.device = int(device)
        self._create(int(d), self.device)

    @classmethod
    def from_triples(cls, triples, resolution, n_bins, device, want_regions=False):
        """Scatter (n, 3) rows [pos_i, pos_j, count].  With want_regions also returns
        `numpy.union1d(pos_i, pos_j)` (pyx:120): when every position is exactly
        bin * resolution -- Rao's format -- it is the bins the scatter kernel saw times the
        resolution (no sort of 2n doubles on the host); otherwise numpy's own union1d."""
        # numpy.nan_to_num (pyx:102) is applied by the scatter kernels to the values they read:
        # no pass over the triples on the host
        t, buf, row_major = triples_buffer(triples)
        d = int(n_bins) + 1
        self = cls(d, device)                                               # zeros, pyx:99
        present = numpy.zeros(d, dtype=numpy.uint8)
        on_grid = _lib.c_i32(0)
        self._call("scatter_ex", _lib.as_f64_ptr(buf), t.shape[0], int(resolution), row_major,
                   present.ctypes.data_as(_lib.p_u8), on_grid)
        if not want_regions:
            return self
        if on_grid.value:
            regions = numpy.flatnonzero(present).astype(numpy.float64) * float(int(resolution))
        else:
            regions = numpy.union1d(_nan_to_num(t[:, 0]), _nan_to_num(t[:, 1]))
        return self, regions

    @classmethod
    def from_host(cls, matrix, device):
        m = numpy.ascontiguousarray(matrix, dtype=numpy.float64)
        self = cls(m.shape[0], device)
        self._call("upload", _lib.as_f64_ptr(m), m.shape[1])
        return self

    @property
    def d(self):
        return int(self._get(_lib.c_i64, "dim"))

    def to_host(self):
        d = self.d
        out = numpy.empty((d, d), dtype=numpy.float64)
        if d:
            self._call("download", _lib.as_f64_ptr(out), d)
        return out


def check_balance_args(ignore_diags=0, min_nnz=0, tol=1e-5, max_iter=200, row_sum=None):
    """The arguments `ContactMap.balance`, `DeviceTriples.balance` and `balance_triples` share,
    converted and checked (ValueError) without touching the library."""
    import math
    ignore_diags, min_nnz, max_iter = int(ignore_diags), int(min_nnz), int(max_iter)
    tol = float(tol)
    if ignore_diags < 0 or min_nnz < 0:
        raise ValueError("ignore_diags and min_nnz must not be negative")
    if not (tol >= 0.0 and math.isfinite(tol)):
        raise ValueError("tol must be finite and not negative")
    if max_iter < 0:
        raise ValueError("max_iter must not be negative")
    if row_sum is not None and not (float(row_sum) > 0.0 and math.isfinite(float(row_sum))):
        raise ValueError("row_sum must be positive and finite")
    return ignore_diags, min_nnz, tol, max_iter, row_sum


_COARSEN_HOW = {"sum": _lib.BB_COARSEN_SUM, "mean": _lib.BB_COARSEN_MEAN}


def check_coarsen_args(factor, how="sum"):
    """(factor, how code) of `ContactMap.coarsen`, `DeviceTriples.coarsen` and `coarsen_triples`,
    checked (ValueError) without touching the library: an int >= 1 -- no bool, no float -- and
    'sum' or 'mean'."""
    factor = check_factor(factor)
    if not isinstance(how, str) or how not in _COARSEN_HOW:
        raise ValueError("how must be 'sum' or 'mean'")
    return factor, _COARSEN_HOW[how]


def expected_from_sums(sums, counts):
    """e[k] = sums[k] / counts[k], NaN where counts[k] == 0 or sums[k] == 0 (docs/SPEC.md 2.5.2)."""
    sums = numpy.asarray(sums, dtype=numpy.float64)
    ok = (numpy.asarray(counts) > 0) & (sums != 0.0)
    e = numpy.full(sums.shape, numpy.nan)
    e[ok] = sums[ok] / numpy.asarray(counts)[ok]
    return e


def _balance(target, n, args):
    """`ContactMap.balance` and `DeviceTriples.balance` in one: the ICE bias of `target`'s map
    over bins 0 .. n - 1 (`bb_cm_balance` / `bb_triples_balance`, whichever handle
    `target._balance_target()` is) under `args`, the tuple `check_balance_args` returned; the
    four `balance_*_` attributes are left on `target`."""
    ignore_diags, min_nnz, tol, max_iter, row_sum = args
    bias = numpy.empty(n, dtype=numpy.float64)
    masked = numpy.zeros(n, dtype=numpy.uint8)
    it, var = _lib.c_i64(), _lib.c_dbl()
    target._balance_target()._call(
        "balance", n, ignore_diags, min_nnz, tol, max_iter, 0.0 if row_sum is None else float(row_sum),
        _lib.as_f64_ptr(bias), masked.ctypes.data_as(_lib.p_u8), it, var)
    target.balance_iterations_, target.balance_variance_ = int(it.value), float(var.value)
    target.balance_converged_ = target.balance_variance_ < tol
    target.balance_masked_ = masked.astype(bool)
    return bias


def expected_sums(dev, n, bias=None):
    """(sums, counts) per distance k = 0 .. n - 1 of the handle `dev`'s map divided by
    bias[i] bias[j] (`bb_cm_expected` / `bb_triples_expected`; None: all ones)."""
    sums = numpy.zeros(n, dtype=numpy.float64)
    counts = numpy.zeros(n, dtype=numpy.int64)
    dev._call("expected", n, None if bias is None else _lib.as_f64_ptr(bias), _lib.as_f64_ptr(sums),
              counts.ctypes.data_as(_lib.p_i64))
    return sums, counts


def _expected(target, n, bias):
    """`ContactMap.expected` and `DeviceTriples.expected` in one: the expected of `target`'s map
    over bins 0 .. n - 1 under `bias` (None or n values); `expected_sums_` and
    `expected_counts_` are left on `target`."""
    if bias is not None:
        bias = numpy.ascontiguousarray(bias, dtype=numpy.float64)
        if bias.shape != (n,):
            raise ValueError("bias must have n_bins = %d values, got shape %r" % (n, bias.shape))
    sums, counts = expected_sums(target._balance_target(), n, bias)
    target.expected_sums_, target.expected_counts_ = sums, counts
    return expected_from_sums(sums, counts)


def check_insulation_args(window, ignore_diags=2, min_valid=0.66):
    """(window, ignore_diags, min_valid) of `ContactMap.insulation`, `DeviceTriples.insulation` and
    `insulation_triples`, checked (ValueError) without touching the library: an int >= 1, an
    int >= 0 -- no bool, no float -- and a share in [0, 1]."""
    def whole(v):
        return isinstance(v, (int, numpy.integer)) and not isinstance(v, bool)
    if not whole(window) or int(window) < 1:
        raise ValueError("window must be an int >= 1")
    if not whole(ignore_diags) or int(ignore_diags) < 0:
        raise ValueError("ignore_diags must be an int >= 0")
    min_valid = float(min_valid)
    if not 0.0 <= min_valid <= 1.0:
        raise ValueError("min_valid must be in [0, 1]")
    return int(window), int(ignore_diags), min_valid


def insulation_full_cells(window, ignore_diags):
    """The cells of an unclipped diamond: window^2 less the cells nearer the diagonal than
    `ignore_diags` -- offset k = b - a has k + 1 cells up to window - 1 and 2 window - 1 - k above
    (docs/SPEC.md 2.13; window 10, ignore_diags 2: 97)."""
    w = int(window)
    k = numpy.arange(min(int(ignore_diags), 2 * w - 1), dtype=numpy.int64)
    return w * w - int(numpy.where(k <= w - 1, k + 1, 2 * w - 1 - k).sum())


def _local_maxima(x):
    """`scipy.signal.find_peaks(x)[0]` of a NaN-free vector: the samples higher than both
    neighbours, a plateau once at floor((l + r) / 2); an end sample, or a plateau that reaches
    one, never."""
    n = x.shape[0]
    change = numpy.flatnonzero(x[1:] != x[:-1]) + 1          # where a new plateau starts
    starts = numpy.concatenate([numpy.zeros(1, dtype=numpy.int64), change])
    ends = numpy.concatenate([change, numpy.full(1, n, dtype=numpy.int64)]) - 1
    v = x[starts]
    k = numpy.flatnonzero((v[1:-1] > v[:-2]) & (v[1:-1] > v[2:])) + 1
    return ((starts[k] + ends[k]) // 2).astype(numpy.int64)


def _nearest_higher_left(x):
    """L[i]: the nearest j < i with x[j] > x[i], -1 where there is none.  Pointer jumping: nothing
    between L[i] and i is higher than x[i] at any time, so a candidate that is not higher is
    replaced by its own candidate -- every bin at once, a few passes."""
    L = numpy.arange(-1, x.shape[0] - 1)
    todo = numpy.flatnonzero(L >= 0)
    while todo.shape[0]:
        todo = todo[x[L[todo]] <= x[todo]]
        L[todo] = L[L[todo]]
        todo = todo[L[todo] >= 0]
    return L


def _prominences(x, peaks):
    """`scipy.signal.peak_prominences(x, peaks)[0]` of a NaN-free vector: from each peak out to
    the nearest higher sample on either side (or the end), the lowest sample of each stretch;
    the peak less the higher of the two.  Comparisons and one subtraction."""
    n = x.shape[0]
    if peaks.shape[0] == 0:
        return numpy.zeros(0)
    first = _nearest_higher_left(x)[peaks] + 1                        # the left stretch is [first, peak]
    end = n - 1 - _nearest_higher_left(x[::-1])[n - 1 - peaks]        # the right one [peak, end)
    xs = numpy.append(x, numpy.inf)                                   # (so that end = n is an index)
    left = numpy.minimum.reduceat(xs, numpy.stack([first, peaks + 1], axis=1).ravel())[::2]
    right = numpy.minimum.reduceat(xs, numpy.stack([peaks, end], axis=1).ravel())[::2]
    return x[peaks] - numpy.maximum(left, right)


class InsulationTrack(object):
    """The insulation score of a map along its diagonal and its domain boundaries (docs/SPEC.md
    2.13), from the two vectors the device leaves -- `sums` (float64) and `counts` (int64) of the
    live cells of every bin's diamond of `window` bins, cells nearer the diagonal than
    `ignore_diags` left out.  Host numpy, O(n_bins); needs no device.

    sums, counts    as given
    full_cells      the cells of an unclipped diamond
    score           sums / counts; NaN where counts is 0 or below min_valid * full_cells
    log2            log2(score / mean), the mean over the finite positive scores; NaN where the
                    score is NaN or <= 0
    strength        the boundary strength -- the prominence of the minimum of `log2` within its
                    maximal run of finite values (`scipy.signal.find_peaks` and `peak_prominences`
                    of the negated run, bit for bit) -- at the bins that are local minima, NaN
                    elsewhere; a plateau counts once, in its middle; the ends of a run never
    kernel_ms       the ms of the kernel that made `sums`, by HIP events (0.0 if not given)"""

    def __init__(self, sums, counts, window, ignore_diags, n_bins, resolution, min_valid=0.66,
                 kernel_ms=0.0):
        self.window, self.ignore_diags, self.min_valid = check_insulation_args(window, ignore_diags, min_valid)
        self.n_bins, self.resolution, self.kernel_ms = int(n_bins), int(resolution), float(kernel_ms)
        self.sums = numpy.asarray(sums, dtype=numpy.float64)
        self.counts = numpy.asarray(counts, dtype=numpy.int64)
        if self.sums.shape != (self.n_bins,) or self.counts.shape != (self.n_bins,):
            raise ValueError("sums and counts must have n_bins = %d values" % self.n_bins)
        self.full_cells = insulation_full_cells(self.window, self.ignore_diags)
        ok = (self.counts > 0) & (self.counts >= self.min_valid * self.full_cells)
        self.score = numpy.full(self.n_bins, numpy.nan)
        with numpy.errstate(invalid="ignore", over="ignore"):
            self.score[ok] = self.sums[ok] / self.counts[ok]
            good = numpy.isfinite(self.score) & (self.score > 0.0)
            self.log2 = numpy.full(self.n_bins, numpy.nan)
            if good.any():
                self.log2[good] = numpy.log2(self.score[good] / self.score[good].mean())
        self.strength = numpy.full(self.n_bins, numpy.nan)
        finite = numpy.isfinite(self.log2)
        edge = numpy.flatnonzero(numpy.diff(numpy.concatenate([[False], finite, [False]]).astype(numpy.int8)))
        for lo, hi in zip(edge[::2], edge[1::2]):            # the maximal runs [lo, hi) of finite log2
            x = -self.log2[lo:hi]
            peaks = _local_maxima(x)
            self.strength[lo + peaks] = _prominences(x, peaks)

    def boundaries(self, min_strength=0.0):
        """(bins, strengths): the local minima of `log2` whose strength is at least
        `min_strength`, bins int64 ascending."""
        with numpy.errstate(invalid="ignore"):
            bins = numpy.flatnonzero(self.strength >= float(min_strength)).astype(numpy.int64)
        return bins, self.strength[bins]


def _insulation(target, n, args, bias, resolution):
    """`ContactMap.insulation` and `DeviceTriples.insulation` in one: the track of `target`'s map
    over bins 0 .. n - 1 under `args`, the tuple `check_insulation_args` returned, and `bias`
    (None or n values), by `bb_cm_insulation` / `bb_triples_insulation`."""
    window, ignore_diags, min_valid = args
    if bias is not None:
        bias = numpy.ascontiguousarray(bias, dtype=numpy.float64)
        if bias.shape != (n,):
            raise ValueError("bias must have n_bins = %d values, got shape %r" % (n, bias.shape))
    dev = target._balance_target()
    sums = numpy.zeros(n, dtype=numpy.float64)
    counts = numpy.zeros(n, dtype=numpy.int64)
    dev._call("insulation", n, window, ignore_diags, None if bias is None else _lib.as_f64_ptr(bias),
              _lib.as_f64_ptr(sums), counts.ctypes.data_as(_lib.p_i64))
    return InsulationTrack(sums, counts, window, ignore_diags, n, resolution, min_valid,
                           dev._get(_lib.c_dbl, "insulation_timing"))


class EigenNoConvergence(RuntimeError):
    """`ContactMap.eigenvector` used up `max_matvecs` before its residual reached the
    tolerance (the counterpart of scipy's ArpackNoConvergence, which the reference's
    `eigsh` call raises, `blueberry/datatypes.pyx:234`).  `.eigenvalue`, `.eigenvector`:
    the pair found so far."""

    def __init__(self, msg, eigenvalue, eigenvector):
        RuntimeError.__init__(self, msg)
        self.eigenvalue, self.eigenvector = eigenvalue, eigenvector


class ContactMap(object):
    """This is a contact map for Hi-C datasets.

    Same parameters and attributes as the reference class
    (`blueberry/datatypes.pyx:31-76`).

    Parameters
    ----------
    celltype : str
    chromosome : int
    resolution : int

    Attributes
    ----------
    resolution, chromosome, celltype, filename, n_bins
    matrix : numpy.ndarray, shape=(n_bins+1, n_bins+1), float64
    regions : numpy.ndarray -- the midpoints found in this map

    Where the matrix lives.  The reference keeps one host matrix alive across
    `__init__` -> `normalize()` -> `filter()` -> consumer (pyx:97-120, :161-171,
    :140-141).  Here that one matrix lives in HBM (`bb_cm_*`, include/blueberry_hip.h):
    the constructor scatters the triples on the device, `normalize()` and `filter()`
    work on the resident matrix in place, and `StructureSolver.fit(contact_map)` packs
    it device to device -- no (n_bins+1)^2 host transfer anywhere on that path.
    `matrix` is fetched lazily and is a READ-ONLY copy while the matrix lives in HBM: a read
    does not cost the residency.  `to_host()` returns a private writable copy and leaves the
    device copy authoritative; `host_matrix()` / `cm.matrix = m` make a host array the
    authoritative one.  `device=None` means this rank's own GPU inside a torch.distributed
    job (LOCAL_RANK, as `StructureSolver` picks it), else device 0.
    """

    def __init__(self, celltype, chromosome, resolution=1000, device=None):
        import pandas
        self.resolution = int(resolution)
        self.chromosome = chromosome
        self.celltype = celltype
        self.device = pick_device(device, several_ranks())
        kb = self.resolution // 1000
        self.filename = RAW_DIR.format(celltype, chromosome, kb)
        self._KRnorm = numpy.atleast_1d(numpy.loadtxt(KR_NORM.format(celltype, chromosome, kb)))
        self._KRexpected = numpy.atleast_1d(numpy.loadtxt(KR_EXP.format(celltype, chromosome, kb)))
        self.n_bins = int(self._KRnorm.shape[0])
        data = pandas.read_csv(self.filename, delimiter="\t", engine="c", dtype="float64",
                               header=None).values               # nan_to_num: on the device
        self._host = self._view = None
        self._dev, self.regions = _DeviceMatrix.from_triples(data, self.resolution, self.n_bins,
                                                             self.device, want_regions=True)
        self.regions.sort()

    # -- where the matrix lives ------------------------------------------
    @property
    def matrix(self):
        """The (n_bins+1)^2 float64 matrix.  While the matrix lives in HBM this is a
        READ-ONLY host copy (fetched once, dropped when a device operation changes the
        matrix): looking at `cm.matrix.shape`, `.sum()` or a cell costs one download, not
        the residency.  Round 2 handed out a writable array and, because the caller might
        write into it, gave the device copy up on every read -- 5 GB down and 5 GB up again
        around a `cm.matrix[0, 0]` at chr1@10kb.  To CHANGE the matrix assign a new one
        (`cm.matrix = m`) or ask for the writable host copy (`cm.host_matrix()`); both
        make the host array the authoritative one, as the reference's attribute is
        (`blueberry/datatypes.pyx:85`)."""
        if self._dev is None:
            return self._host
        if self._view is None:
            v = self._dev.to_host()
            v.flags.writeable = False
            self._view = v
        return self._view

    @matrix.setter
    def matrix(self, value):
        self._host = value
        self._view = None
        if self._dev is not None:
            self._dev.close()
            self._dev = None

    def host_matrix(self):
        """The matrix as a writable host array that is from now on the authoritative copy
        (the resident one is given up; the next device operation uploads the array again)."""
        if self._dev is not None:
            self._host = self._dev.to_host()
            self._dev.close()
            self._dev = None
        self._view = None
        return self._host

    def to_host(self):
        """A private copy of the matrix; the resident one stays authoritative."""
        if self._dev is not None:
            return self._dev.to_host()
        return numpy.array(self._host, dtype=numpy.float64)

    @property
    def is_resident(self):
        """True while the authoritative matrix is the one in HBM."""
        return self._dev is not None

    def _resident(self):
        """The device handle of the authoritative matrix (uploading a host one)."""
        if self._dev is None:
            m = numpy.ascontiguousarray(self._host, dtype=numpy.float64)
            if m.ndim != 2 or m.shape[0] != m.shape[1]:
                raise ValueError("matrix must be square")
            if m.shape[0] == 0:
                raise ValueError("the contact map is empty (every bin was filtered out)")
            self._dev = _DeviceMatrix.from_host(m, self.device)
            self._host = None
        self._view = None      # the caller is about to work on (usually: change) the resident matrix
        return self._dev

    # a ContactMap pickles / deep-copies as its host matrix: the device handle is a pointer
    # into this process's HIP context and means nothing anywhere else
    def __getstate__(self):
        state = dict(self.__dict__)
        state["_host"] = self.to_host()
        state["_dev"] = state["_view"] = None
        return state

    def __setstate__(self, state):
        self.__dict__.update(state)

    @property
    def shape(self):
        d = self._dev.d if self._dev is not None else self._host.shape[0]
        return (d, d)

    # ------------------------------------------------------------------
    @classmethod
    def from_arrays(cls, celltype, chromosome, resolution, contacts, n_bins=None, KRnorm=None,
                    KRexpected=None, symmetric=True, device=None):
        """Create a contact map from numpy arrays.  No files required.

        contacts : (n, 3) array of (mid1, mid2, statistic), mid = bin midpoint,
        placed at bin int((mid - resolution/2) / resolution) as at
        `blueberry/datatypes.pyx:268-271`.  `symmetric` also sets the mirrored
        cell (the file constructor's matrices are symmetric; the reference's
        from_arrays would have set one triangle only)."""
        self = cls.__new__(cls)
        self.resolution = int(resolution)
        self.chromosome = chromosome
        self.celltype = celltype
        self.device = pick_device(device, several_ranks())
        self.filename = ""
        contacts = numpy.asarray(contacts, dtype=numpy.float64)
        if contacts.ndim != 2 or contacts.shape[1] != 3:
            raise ValueError("contacts must have shape (n, 3)")
        b1 = ((contacts[:, 0] - self.resolution / 2.0) / self.resolution).astype(numpy.int64)
        b2 = ((contacts[:, 1] - self.resolution / 2.0) / self.resolution).astype(numpy.int64)
        if n_bins is None:
            n_bins = (KRnorm.shape[0] if KRnorm is not None
                      else int(max(b1.max(initial=-1), b2.max(initial=-1)) + 1))
        self.n_bins = int(n_bins)
        if contacts.shape[0] and (min(b1.min(), b2.min()) < 0 or
                                  max(b1.max(), b2.max()) > self.n_bins):
            raise ValueError("a contact falls outside [0, n_bins]")
        d = self.n_bins + 1
        m = numpy.zeros((d, d), dtype=numpy.float64)
        if symmetric:
            # the reference's order of stores: [b1, b2] then [b2, b1], entry by entry
            rows = numpy.stack([b1, b2], axis=1).reshape(-1)
            cols = numpy.stack([b2, b1], axis=1).reshape(-1)
            _assign_last_wins(m, rows, cols, numpy.repeat(contacts[:, 2], 2))
        else:
            _assign_last_wins(m, b1, b2, contacts[:, 2])     # later rows win, as in the reference
        self._host, self._dev, self._view = m, None, None
        self.regions = numpy.union1d(contacts[:, 0], contacts[:, 1])
        self._KRnorm = None if KRnorm is None else numpy.asarray(KRnorm, dtype=numpy.float64)
        self._KRexpected = (None if KRexpected is None
                            else numpy.asarray(KRexpected, dtype=numpy.float64))
        return self

    @classmethod
    def from_matrix(cls, matrix, resolution=1000, celltype="", chromosome=0, KRnorm=None,
                    KRexpected=None, device=None):
        """Wrap an existing dense symmetric ((n_bins+1)^2) float64 matrix."""
        self = cls.__new__(cls)
        m = numpy.ascontiguousarray(matrix, dtype=numpy.float64)
        if m.ndim != 2 or m.shape[0] != m.shape[1] or m.shape[0] < 1:
            raise ValueError("matrix must be square")
        self.resolution, self.chromosome, self.celltype = int(resolution), chromosome, celltype
        self.device, self.filename = pick_device(device, several_ranks()), ""
        self._host, self._dev, self._view = m, None, None
        self.n_bins = m.shape[0] - 1
        self.regions = numpy.arange(self.n_bins, dtype=numpy.float64) * self.resolution
        self._KRnorm = None if KRnorm is None else numpy.asarray(KRnorm, dtype=numpy.float64)
        self._KRexpected = (None if KRexpected is None
                            else numpy.asarray(KRexpected, dtype=numpy.float64))
        return self

    @classmethod
    def from_triples(cls, triples, resolution, n_bins, KRnorm=None, KRexpected=None, celltype="",
                     chromosome=0, device=None):
        """The file constructor without the files: Rao-format (n, 3) rows
        [pos_i, pos_j, count] (what `__init__` reads, pyx:100-102), scattered on the
        device; the matrix is never built on the host."""
        self = cls.__new__(cls)
        self.resolution, self.chromosome, self.celltype = int(resolution), chromosome, celltype
        self.device, self.filename = pick_device(device, several_ranks()), ""
        data = numpy.asarray(triples, dtype=numpy.float64)         # nan_to_num: on the device
        self.n_bins = int(n_bins)
        self._host = self._view = None
        self._dev, self.regions = _DeviceMatrix.from_triples(data, self.resolution, self.n_bins,
                                                             self.device, want_regions=True)
        self._KRnorm = None if KRnorm is None else numpy.asarray(KRnorm, dtype=numpy.float64)
        self._KRexpected = (None if KRexpected is None
                            else numpy.asarray(KRexpected, dtype=numpy.float64))
        return self

    # ------------------------------------------------------------------
    def marginals(self):
        """`matrix.sum(axis=0)` of the resident matrix (pyx:140), bit for bit."""
        if self.shape[0] == 0:
            return numpy.zeros(0)
        dev = self._resident()
        out = numpy.empty(dev.d, dtype=numpy.float64)
        dev._call("marginals", _lib.as_f64_ptr(out))
        return out

    def filter(self, threshold=0, keep_stale=False):
        """Remove rows and columns whose marginal count is <= threshold.

        In place, returns None (`blueberry/datatypes.pyx:122-141`); runs on the GPU on
        the resident matrix: column sums in numpy's summation order, prefix-sum
        compaction, gather."""
        if self.shape[0] == 0:
            return                     # nothing left to filter (numpy: an empty index list)
        dev = self._resident()
        d = dev.d
        keep = numpy.zeros(d, dtype=numpy.uint8)
        dn = _lib.c_i64()
        dev._call("filter", float(threshold), dn, keep.ctypes.data_as(_lib.p_u8))
        keep = keep.astype(bool)
        if not keep_stale:
            # bins that survive, in the old numbering; the zero padding row
            # (index n_bins) never survives threshold >= 0
            self.n_bins = int(dn.value)
            if self.regions is not None and self.regions.shape[0]:
                bins = (self.regions / self.resolution).astype(numpy.int64)
                ok = (bins >= 0) & (bins < keep.shape[0])
                ok[ok] = keep[bins[ok]]
                self.regions = self.regions[ok]
            # KR vectors describe the unfiltered map: normalize() first, then filter()
            self._KRnorm = None
            self._KRexpected = None
            # and so do what balance() / expected() left beside them
            self.balance_masked_ = None
            self.expected_sums_ = self.expected_counts_ = None

    def normalize(self):
        """KR matrix balancing and observed/expected normalisation, in place.

        m[j, j+i] /= KRnorm[j] * KRnorm[j+i] * KRexpected[i], mirrored, then
        nan_to_num (`blueberry/datatypes.pyx:143-171`); runs on the GPU on the
        resident matrix."""
        if self._KRnorm is None or self._KRexpected is None:
            raise ValueError("normalize() needs KRnorm and KRexpected")
        n = self.n_bins
        if self.shape != (n + 1, n + 1):
            raise ValueError("matrix shape does not match n_bins (was filter() used with "
                             "keep_stale=True?)")
        if self._KRnorm.shape[0] < n or self._KRexpected.shape[0] < n:
            raise ValueError("KRnorm / KRexpected shorter than n_bins")
        kr = numpy.ascontiguousarray(self._KRnorm[:n], dtype=numpy.float64)
        ke = numpy.ascontiguousarray(self._KRexpected[:n], dtype=numpy.float64)
        if n and (numpy.any(kr == 0.0) or numpy.any(ke == 0.0)):
            raise ZeroDivisionError("float division")
        self._resident()._call("normalize", n, _lib.as_f64_ptr(kr), _lib.as_f64_ptr(ke))

    # -- balancing a raw map (docs/SPEC.md 2.5.2) --------------------------
    def _balance_target(self):
        """The device handle for balance() / expected(), which read the leading n_bins x n_bins
        block and leave the matrix as it is (a host copy handed out by `matrix` stays valid)."""
        n = self.n_bins
        if self.shape[0] == 0:
            raise ValueError("the contact map is empty (every bin was filtered out)")
        if self.shape != (n + 1, n + 1):
            raise ValueError("matrix shape does not match n_bins (was filter() used with "
                             "keep_stale=True?)")
        return self._dev if self._dev is not None else self._resident()

    def _divide(self, bias, expected):
        """The existing normalize path with the two vectors given (the map's own stay)."""
        keep = self._KRnorm, self._KRexpected
        self._KRnorm, self._KRexpected = bias, expected
        try:
            self.normalize()
        finally:
            self._KRnorm, self._KRexpected = keep

    def balance(self, ignore_diags=0, min_nnz=0, tol=1e-5, max_iter=200, row_sum=None, apply=False):
        """The bias vector of iterative correction (ICE; Imakaev et al. 2012) of the raw map,
        computed on the resident matrix (`bb_cm_balance`; the definition is docs/SPEC.md 2.5.2).

        The counted cells are those of the bins 0 .. n_bins - 1 with |i - j| >= `ignore_diags`.
        A bin is masked if it has fewer than `min_nnz` non-zero counted cells or no count in
        common with an unmasked bin.  The loop stops when the variance of the live bins' row sums,
        relative to their mean, is below `tol`, or after `max_iter` updates.  The vector is scaled
        so that the balanced map's mean row sum is `row_sum` -- None: the raw map's, so that the
        counts keep their magnitude; 1.0: cooler's convention.

        Returns the length-n_bins float64 vector b, NaN at masked bins (as Rao's KRnorm files
        mark them), and keeps it as the map's KRnorm, so that `normalize()` and `fit_triples(
        KRnorm=...)` can use it.  Sets `balance_iterations_` (updates made), `balance_variance_`,
        `balance_converged_` and `balance_masked_` (bool array).  A negative or non-finite counted
        cell raises ValueError.  apply=False leaves the matrix as it is, bit for bit; apply=True
        then divides it in place by b_i b_j (`normalize()` with an all-ones expected vector:
        masked bins become 0).  The same bits on every run."""
        args = check_balance_args(ignore_diags, min_nnz, tol, max_iter, row_sum)
        self._KRnorm = bias = _balance(self, self.n_bins, args)
        if apply:
            self._divide(bias, numpy.ones(self.n_bins))
        return bias

    def _bias_argument(self, bias):
        """The `bias` of `expected()` and `insulation()`: 'auto' -- the map's KRnorm, cut to n_bins
        values, or None if there is none; anything else as it is."""
        if not isinstance(bias, str):
            return bias
        if bias != "auto":
            raise ValueError("bias must be 'auto', None or a vector of n_bins values")
        if self._KRnorm is None:
            return None
        if self._KRnorm.shape[0] < self.n_bins:
            raise ValueError("KRnorm shorter than n_bins")
        return self._KRnorm[:self.n_bins]

    def expected(self, bias="auto", apply=False):
        """The distance-decay expected of the balanced map: e[k] = the mean over the live pairs
        at distance k of M[i, i+k] / (bias[i] bias[i+k]), k = 0 .. n_bins - 1, in one sweep of the
        resident upper triangle (`bb_cm_expected`; docs/SPEC.md 2.5.2).  A pair with a NaN bias
        is not a live pair.  e[k] is NaN where no live pair exists or their sum is 0 -- never 0 --
        so that `normalize()` turns such cells into 0.

        `bias`: 'auto' -- the map's KRnorm (what `balance()` left, or what the constructor was
        given) if there is one, else all ones; None -- all ones; or a length-n_bins vector.
        Returns e and keeps it as the map's KRexpected; `expected_sums_` and `expected_counts_`
        (int64) hold the two raw vectors.  apply=True then divides the map in place by
        e[|i - j|] alone (`normalize()` with an all-ones bias).  After `balance()` and
        `expected()` without `apply`, `normalize()` applies both, as on a Rao map."""
        n = self.n_bins
        self._KRexpected = _expected(self, n, self._bias_argument(bias))
        if apply:
            self._divide(numpy.ones(n), self._KRexpected)
        return self._KRexpected

    def significance(self, **kwargs):
        """The Fit-Hi-C p- and q-values of this raw map's contacts as a `FithicContactMap`
        (docs/SPEC.md 2.9): `FitHiC(resolution=self.resolution, **kwargs).fit_transform(self)`,
        with `biases` ('auto': the map's KRnorm, e.g. what `balance()` left) and `q_max` (only the
        contacts with q <= q_max, selected on the device) passed on to `fit_transform`.  The map
        stays as it is and stays resident."""
        from .fithic import _significance      # (late: fithic takes this very type -- a real cycle)
        return _significance(self, None, kwargs)

    def correlation(self):
        """Convert the map to a correlation map, in place (pyx:173-188:
        `numpy.corrcoef(matrix)`), on the resident matrix: rows centred, Gram matrix on
        the fp64 matrix cores, scaled by the diagonal and clipped to [-1, 1] in numpy's
        order of operations (`bb_cm_correlation`).  Equal to numpy to rounding.
        `correlation_tflops_` holds the rate of the Gram kernel afterwards."""
        if self.shape[0] == 0:
            return
        dev = self._resident()
        self.correlation_tflops_ = float(dev._get(_lib.c_dbl, "correlation"))

    def shortest_paths(self, alpha=3.0, kind="counts"):
        """Complete the map by graph shortest paths (docs/SPEC.md 2.1.1; ShRec3D, Isomap): a
        NEW ContactMap (same celltype, chromosome, resolution, regions, n_bins; no KR vectors)
        whose resident matrix is G, G_ij = the length of the shortest chain of wish distances
        between bins i and j -- `count ** (-1 / alpha)` of every finite positive count for
        kind='counts', the entries themselves for kind='wish' -- with a 0 diagonal and 0 ("no
        constraint") where no chain exists (dead bins, separate components);
        `unreachable_pairs_` counts those pairs.  G is a kind='wish' input for
        `StructureSolver`.  A measured pair may get shorter: G is the metric closure.  Blocked
        Floyd-Warshall on the device in float64 (`bb_cm_shortest_paths`), the same bits on
        every run.  This map is left as it is and stays resident.

        The work matrix is a second matrix-sized allocation (5 GB at chr1@10kb; freed by
        `bb_cm_release_scratch`).  A whole-genome map that is only ever held blocked-sparse
        (720 GB dense at 10 kb) cannot be completed this way: the allocation fails with
        MemoryError."""
        kind_code, alpha = _completion_arguments(kind, alpha)
        if self.shape[0] == 0:
            raise ValueError("the contact map is empty (every bin was filtered out)")
        src = self._dev if self._dev is not None else self._resident()
        out = ContactMap.__new__(ContactMap)
        out.resolution, out.chromosome, out.celltype = self.resolution, self.chromosome, self.celltype
        out.device, out.filename, out.n_bins = src.device, self.filename, self.n_bins
        out.regions = None if self.regions is None else numpy.array(self.regions)
        out._KRnorm = out._KRexpected = None
        out._host = out._view = None
        out._dev = _DeviceMatrix(src.d, src.device)
        out.unreachable_pairs_ = _shortest_paths_device(src, out._dev, kind_code, alpha)
        return out

    def coarsen(self, factor, how="sum"):
        """The map pooled to resolution `resolution * factor` (docs/SPEC.md 2.12): a NEW resident
        ContactMap of `ceil(n_bins / factor)` bins (same celltype, chromosome and device; no KR
        vectors, nothing of `balance()` / `expected()`), computed on the device from the upper
        triangle of the leading n_bins x n_bins block (`bb_cm_coarsen`).  Coarse bin I holds the
        fine bins [I factor, (I + 1) factor) -- the last may be ragged; cell (I, J) is the sum of
        its block, (I, I) the sum of the block's upper triangle with the diagonal (every fine pair
        once: the contacts inside the bin, cooler's convention).  how='mean' divides by the
        number of fine cells pooled, zero cells included -- for O/E-normalised maps.  `regions`
        are the old ones rounded down to the new grid.  Float64 in a fixed order of summation: the
        same bits on every run, and the bits `coarsen_triples` gives from the pixel list.  This
        map is left as it is and stays resident; a filtered map (its edge is no longer
        n_bins + 1) is refused."""
        factor, how = check_coarsen_args(factor, how)
        src = self._balance_target()
        n = self.n_bins
        nc = -(-n // factor)
        out = ContactMap.__new__(ContactMap)
        out.resolution = self.resolution * factor
        out.chromosome, out.celltype = self.chromosome, self.celltype
        out.device, out.filename, out.n_bins = src.device, self.filename, nc
        if self.regions is None:
            out.regions = None
        else:
            R = float(out.resolution)
            out.regions = numpy.unique(numpy.floor(numpy.asarray(self.regions, dtype=numpy.float64) / R) * R)
        out._KRnorm = out._KRexpected = None
        out._host = out._view = None
        out._dev = _DeviceMatrix(nc + 1, src.device)
        src._call("coarsen", n, factor, how, out._dev._open())
        return out

    def insulation(self, window, ignore_diags=2, bias="auto", min_valid=0.66):
        """The insulation score of the map and its domain (TAD) boundaries as an `InsulationTrack`
        (docs/SPEC.md 2.13; Crane et al. 2015, cooltools' convention): per bin i the sum and the
        number of the live cells of the diamond of `window` bins whose corner sits on (i, i) --
        rows i - window + 1 .. i, columns i .. i + window - 1, clipped to the map, the cells
        nearer the diagonal than `ignore_diags` left out -- each cell divided by bias_a bias_b, in
        one banded pass over the resident upper triangle (`bb_cm_insulation`); score, log2 and
        boundaries follow on the host.  A bin with a NaN bias is not live: its cells are neither
        added nor counted.  A bin whose diamond has fewer than `min_valid` of an unclipped
        diamond's cells gets no score.

        `bias` as in `expected()`: 'auto' -- the map's KRnorm (what `balance()` left, or what the
        constructor was given) if there is one, else all ones; None -- all ones, for a map that
        is balanced already; or a length-n_bins vector.  Float64 in a fixed order of summation:
        the same bits on every run, and the bits `insulation_triples` gives from the pixel list.
        The map is left as it is and stays resident; a filtered map is refused."""
        args = check_insulation_args(window, ignore_diags, min_valid)
        return _insulation(self, self.n_bins, args, self._bias_argument(bias), self.resolution)

    def plot(self, arcsinh=True, **kwargs):
        """Plot the contact map onto the current palette (pyx:190-214)."""
        import matplotlib.pyplot as plt
        plt.title("{} chr{} at {}kb resolution".format(self.celltype, self.chromosome,
                                                       self.resolution // 1000), fontsize=16)
        plt.xlabel("Genomic Coordinate (kb)", fontsize=14)
        plt.ylabel("Genomic Coordinate (kb)", fontsize=14)
        plt.xticks(fontsize=14)
        plt.yticks(fontsize=14)
        m = self.to_host()
        plt.imshow(numpy.arcsinh(m) if arcsinh else m, **kwargs)

    def eigenvector(self, tol=1e-13, max_matvecs=2000):
        """First eigenvector of the matrix (pyx:216-235).

        The reference calls `scipy.sparse.linalg.eigsh(matrix, k=1)`: ARPACK's
        restarted Lanczos for the eigenpair of largest magnitude.  Here the same
        pair comes from a restarted Lanczos over the RESIDENT matrix (`bb_cm_eigenvector`:
        one HBM sweep per matrix-vector product, basis on the device).  ARPACK's sign is
        arbitrary; this one makes the largest-magnitude component positive.
        `eigenvalue_` holds the eigenvalue afterwards."""
        dev = self._resident()
        d = dev.d
        vec = numpy.empty(d, dtype=numpy.float64)
        lam, used, res = _lib.c_dbl(), _lib.c_i64(), _lib.c_dbl()
        dev._call("eigenvector", _lib.as_f64_ptr(vec), lam, float(tol), int(max_matvecs), used, res)
        self.eigenvalue_, self.eigen_matvecs_, self.eigen_residual_ = (
            float(lam.value), int(used.value), float(res.value))
        if self.eigen_residual_ > max(float(tol), 2.3e-16) * abs(self.eigenvalue_):
            # scipy's eigsh raises ArpackNoConvergence here; the unconverged pair travels
            # with the exception as ARPACK's does
            raise EigenNoConvergence(
                "eigenvector: residual %.3e after %d matrix-vector products (tol %.1e x |%.6e|)"
                % (self.eigen_residual_, self.eigen_matvecs_, tol, self.eigenvalue_),
                self.eigenvalue_, vec)
        return vec


_COMPLETION_KINDS = {"wish": _lib.BB_KIND_WISH, "counts": _lib.BB_KIND_COUNTS}


def _completion_arguments(kind, alpha):
    """(kind code, alpha) of a shortest-path completion, checked without a device."""
    if kind not in _COMPLETION_KINDS:
        raise ValueError("kind must be 'counts' or 'wish'")
    if not float(alpha) > 0:
        raise ValueError("alpha must be positive")
    return _COMPLETION_KINDS[kind], float(alpha)


def _shortest_paths_device(src, dst, kind_code, alpha):
    """`bb_cm_shortest_paths` from one _DeviceMatrix into another (or itself); returns the
    number of unreachable pairs."""
    return int(src._get(_lib.c_i64, "shortest_paths", dst._open(), kind_code, alpha))


def _dense_from_any(X):
    """A square float64 host matrix from an ndarray or a scipy.sparse matrix.  Sparse: either
    triangle names a pair, of several entries for one pair the last is kept (as
    `StructureSolver.fit` treats it), the diagonal is dropped, unnamed pairs are 0."""
    if hasattr(X, "tocoo"):
        coo = X.tocoo()
        if coo.shape[0] != coo.shape[1]:
            raise ValueError("contact matrix must be square, got shape %r" % (coo.shape,))
        keep = coo.row != coo.col
        r, c = coo.row[keep].astype(numpy.int64), coo.col[keep].astype(numpy.int64)
        upper = numpy.zeros(coo.shape, dtype=numpy.float64)
        _assign_last_wins(upper, numpy.minimum(r, c), numpy.maximum(r, c), coo.data[keep])
        return upper + upper.T
    m = numpy.ascontiguousarray(X, dtype=numpy.float64)
    if m.ndim != 2 or m.shape[0] != m.shape[1]:
        raise ValueError("contact matrix must be square, got shape %r" % (m.shape,))
    return m


def complete_map(X, kind="counts", alpha=3.0, device=None):
    """The shortest-path completion of `X` as a resident ContactMap (`ContactMap.
    shortest_paths`): X a ContactMap (completed on its own device), a square ndarray or a
    scipy.sparse matrix (uploaded to `device` and completed in place)."""
    kind_code, alpha = _completion_arguments(kind, alpha)
    if isinstance(X, ContactMap):
        return X.shortest_paths(alpha=alpha, kind=kind)
    m = _dense_from_any(X)
    if m.shape[0] < 1:
        raise ValueError("the contact matrix is empty")
    out = ContactMap.from_matrix(m, device=device)
    dev = out._resident()
    out.unreachable_pairs_ = _shortest_paths_device(dev, dev, kind_code, alpha)
    return out


def shortest_paths(X, kind="counts", alpha=3.0, device=None):
    """All-pairs shortest-path lengths G over the graph of `X`'s wish distances
    (docs/SPEC.md 2.1.1), as a host ndarray: X a square ndarray, a ContactMap or a
    scipy.sparse matrix (scattered to a dense matrix, last entry of a pair wins).  0 on the
    diagonal and where no path exists.  Computed on the GPU (`bb_cm_shortest_paths`);
    `device=None`: as `ContactMap` picks it.  The dense matrix and a work matrix of the same
    size must fit on the device."""
    return complete_map(X, kind=kind, alpha=alpha, device=device).to_host()


DATA_DIR = RAO + ("results/Rao-Cell2014/fixedWindowSize/fithic/afterICE/{2}/"
                  "{0}.chr{1}.spline_pass1.res{2}.significances.txt.gz")


class FithicContactMap(object):
    """A contact map which has been processed with Fit-Hi-C.

    Same surface as the reference class (`blueberry/datatypes.pyx:274-388`):
    `map` is an (n_contacts, 5) float64 array of (mid1, mid2, contactCount, p, q)
    read from columns [1, 3, 4, 5, 6] of a `.significances.txt.gz` file (format
    written at `blueberry/fithic.py:411`), `regions` the midpoints seen.  It is
    the on-disk adapter that lets real Fit-Hi-C output feed `StructureSolver`:
    `to_sparse()` gives the scipy matrix `fit()` takes without ever building the
    dense one.

    Deviations: `decimate` uses the integer arithmetic the
    Python 2 reference meant (`(int + res) // res * res - res // 2`) and emits
    rows sorted by (mid1, mid2) instead of in dict order; `to_matrix` takes an
    optional `n_bins` instead of always reading the KRnorm file; `from_array`
    builds a map without a file.
    """

    def __init__(self, celltype, chromosome, resolution=1000):
        import pandas
        self.resolution = int(resolution)
        self.filename = DATA_DIR.format(celltype, chromosome, self.resolution)
        self.chromosome = chromosome
        self.celltype = celltype
        self.map = pandas.read_csv(self.filename, sep="\t", usecols=[1, 3, 4, 5, 6], engine="c",
                                   dtype="float64").values
        self.regions = numpy.union1d(self.map[:, 0], self.map[:, 1])

    @classmethod
    def from_array(cls, map_array, resolution, celltype="", chromosome=0):
        self = cls.__new__(cls)
        m = numpy.array(map_array, dtype=numpy.float64)
        if m.ndim != 2 or m.shape[1] != 5:
            raise ValueError("map must have shape (n_contacts, 5): mid1, mid2, count, p, q")
        self.map, self.resolution = m, int(resolution)
        self.filename, self.celltype, self.chromosome = "", celltype, chromosome
        self.regions = numpy.union1d(m[:, 0], m[:, 1])
        return self

    def decimate(self, resolution=5000):
        """Decimate the map to a lower resolution: midpoints are rounded to the
        coarser grid, counts summed, p-values multiplied, q-values minimised
        (`blueberry/datatypes.pyx:317-339`).  In place, returns None."""
        resolution = int(resolution)
        self.resolution = resolution
        mids = (self.map[:, :2].astype(numpy.int64) + resolution) // resolution * resolution \
            - resolution // 2
        key, first, inv = numpy.unique(mids, axis=0, return_index=True, return_inverse=True)
        # one row per (mid1, mid2) in the order of FIRST occurrence: the reference collects
        # them in a dict (`datatypes.pyx:330-336`), whose order that is
        order = numpy.argsort(first, kind="stable")
        rank = numpy.empty_like(order)
        rank[order] = numpy.arange(order.shape[0])
        key, inv = key[order], rank[inv.ravel()]
        count = numpy.zeros(key.shape[0])
        numpy.add.at(count, inv, self.map[:, 2])
        p = numpy.ones(key.shape[0])
        numpy.multiply.at(p, inv, self.map[:, 3])
        q = numpy.ones(key.shape[0])
        numpy.minimum.at(q, inv, self.map[:, 4])
        self.map = numpy.column_stack([key.astype(numpy.float64), count, p, q])
        self.regions = numpy.union1d(self.map[:, 0], self.map[:, 1])

    def contacts(self):
        """All contacts with a q-value <= Q_LOWER_BOUND, as (mid1, mid2) rows
        (`blueberry/datatypes.pyx:341-350`)."""
        return self.map[self.map[:, 4] <= Q_LOWER_BOUND, :2]

    def _bins(self):
        res = self.resolution
        b1 = ((self.map[:, 0] - res / 2.0) / res).astype(numpy.int64)
        b2 = ((self.map[:, 1] - res / 2.0) / res).astype(numpy.int64)
        return b1, b2

    def _statistic(self, statistic):
        col = {"count": 2, "p": 3, "q": 4}.get(statistic)
        if col is None:
            raise ValueError                     # as the reference (pyx:386)
        return self.map[:, col]

    def to_matrix(self, statistic="count", n_bins=None):
        """Convert the map from column format to a 2d (n_bins+1)^2 matrix holding
        `statistic` at [bin(mid1), bin(mid2)] (one triangle, as the reference
        fills it; `blueberry/datatypes.pyx:352-388`)."""
        vals = self._statistic(statistic)
        if n_bins is None:
            kr = numpy.loadtxt(KR_NORM.format(self.celltype, self.chromosome,
                                              self.resolution // 1000))
            n_bins = numpy.atleast_1d(kr).shape[0]
        d = int(n_bins) + 1
        b1, b2 = self._bins()
        matrix = numpy.zeros((d, d))
        _assign_last_wins(matrix, b1, b2, vals)  # later rows win, as in the reference
        return matrix

    def to_sparse(self, statistic="count", n_bins=None):
        """The same content as a scipy.sparse COO matrix of shape (n_bins+1)^2 --
        what `StructureSolver.fit` takes for blocked-sparse input."""
        import scipy.sparse
        vals = self._statistic(statistic)
        b1, b2 = self._bins()
        if n_bins is None:
            n_bins = int(max(b1.max(initial=0), b2.max(initial=0)))
        d = int(n_bins) + 1
        return scipy.sparse.coo_matrix((vals, (b1, b2)), shape=(d, d))
