"""A Rao-format pixel list on the device: the `DeviceTriples` handle and the `GeodesicRows` its
shortest paths leave, and balancing, pooling and the insulation score of a map straight from its
triples (docs/SPEC.md 2.1.2, 2.5.3, 2.12, 2.13)."""
import contextlib

import numpy

from . import _lib
from .datatypes import (_balance, _expected, _insulation, check_balance_args, check_coarsen_args,
                        check_insulation_args, triples_buffer)
from .engine import _kr_pair
from .plan import _DTYPES, _KINDS, layout_info
from .ranks import pick_device, several_ranks


class DeviceTriples(_lib.Handle):
    """The (n, 3) array [pos_i, pos_j, count] of a Rao-format file -- what
    `ContactMap.__init__` reads (`blueberry/datatypes.pyx:100-102`) -- copied to the device
    once (`bb_triples_*`): nan_to_num, binning and the scatter into the solver's tiles all
    happen there.  C-ordered rows and the reference's column-major array are read in place.

    `balance` and `expected` are `ContactMap.balance` / `ContactMap.expected` on the matrix the
    triples define -- `ContactMap.from_triples(triples, resolution, n_bins)` -- without that
    matrix (docs/SPEC.md 2.5.3): the first call builds an index of the stored cells on the
    device, which stays with the handle."""
    is_triples = True
    prefix = "bb_triples_"

    def __init__(self, triples, resolution, device):
        t, buf, row_major = triples_buffer(triples)
        self.resolution = int(resolution)
        _lib.Handle.__init__(self)
        self.n, self.device = int(t.shape[0]), int(device)
        self._create(_lib.as_f64_ptr(buf), self.n, int(resolution), row_major, self.device)

    @classmethod
    def _adopt(cls, handle, resolution, device):
        """The owner of a `bb_triples` another call left (`bb_triples_coarsen`)."""
        self = cls.__new__(cls)
        _lib.Handle.__init__(self, handle)
        self.resolution, self.device = int(resolution), int(device)
        self.n = int(self._get(_lib.c_i64, "size"))
        return self

    def _balance_target(self):
        """The handle `balance`, `expected` and the significance pass speak to: this one."""
        return self

    def to_host(self):
        """The (n, 3) float64 rows [pos_i, pos_j, count] the handle holds, C-ordered, as they
        were given (`bb_triples_download`)."""
        out = numpy.empty((self.n, 3), dtype=numpy.float64)
        self._call("download", _lib.as_f64_ptr(out))
        return out

    def coarsen(self, n_bins, factor, how="sum"):
        """The pixel list of the map the triples define over bins 0 .. n_bins - 1, pooled to
        resolution `resolution * factor` (`ContactMap.coarsen`; docs/SPEC.md 2.12): a NEW
        `DeviceTriples` on the same device -- nothing goes through the host -- of one triple
        [I R, J R, value] per pooled cell I <= J with at least one stored fine cell (a stored 0
        included), I ascending, then J; `n_bins_` holds ceil(n_bins / factor).  The values are
        bit for bit those of `ContactMap.from_triples(...).coarsen(factor, how)`.  The new handle
        is usable wherever a `DeviceTriples` is and does not depend on this one, which stays as
        it is (the first call builds its index, as `balance` does)."""
        factor, how = check_coarsen_args(factor, how)
        n = _bin_count(n_bins)
        h = _lib.c_void_p()
        self._call("coarsen", n, factor, how, h)
        out = DeviceTriples._adopt(h, self.resolution * factor, self.device)
        out.n_bins_ = -(-n // factor)
        return out

    def tiles(self, n_bins, dtype):
        """(tile_I, tile_J), device order, of the tiles the triples name."""
        nb = layout_info(n_bins, dtype)["n_blocks"]
        present = numpy.zeros((nb, nb), dtype=numpy.uint8)
        self._call("tiles", int(n_bins), _DTYPES[dtype], present.ctypes.data_as(_lib.p_u8), nb)
        tj, ti = numpy.nonzero(present.T)            # J ascending, then I
        return ti.astype(numpy.int32), tj.astype(numpy.int32)

    def pairs(self, n_bins):
        """The number of distinct bin pairs i <= j < n_bins the triples store."""
        return int(self._get(_lib.c_i64, "pairs", int(n_bins)))

    def balance(self, n_bins, ignore_diags=0, min_nnz=0, tol=1e-5, max_iter=200, row_sum=None):
        """The ICE bias vector of the map the triples define over bins 0 .. n_bins - 1
        (`bb_triples_balance`): the arguments, the result (length n_bins, NaN at masked bins)
        and the attributes `balance_iterations_`, `balance_variance_`, `balance_converged_`,
        `balance_masked_` of `ContactMap.balance`.  The same bits on every run, and for every
        duplicate-free list of the same pairs."""
        args = check_balance_args(ignore_diags, min_nnz, tol, max_iter, row_sum)
        return _balance(self, _bin_count(n_bins), args)

    def expected(self, n_bins, bias=None):
        """The distance-decay expected e of the balanced map (`bb_triples_expected`,
        `ContactMap.expected`): bias None -- all ones -- or a length-n_bins vector, NaN = not a
        live bin.  `expected_sums_` and `expected_counts_` (int64) hold the two raw vectors;
        pairs without a triple are zero cells and count."""
        return _expected(self, _bin_count(n_bins), bias)

    def insulation(self, n_bins, window, ignore_diags=2, bias=None, min_valid=0.66):
        """The `InsulationTrack` of the map the triples define over bins 0 .. n_bins - 1
        (`ContactMap.insulation`; docs/SPEC.md 2.13), bit for bit what `ContactMap.from_triples(
        ...).insulation(...)` gives, without that matrix (`bb_triples_insulation`; the first call
        builds the handle's index, as `balance` does).  bias None -- all ones -- or a length-n_bins
        vector, NaN = not a live bin; pairs without a triple are zero cells and count."""
        args = check_insulation_args(window, ignore_diags, min_valid)
        return _insulation(self, _bin_count(n_bins), args, bias, self.resolution)

    def significance(self, map_bins, **kwargs):
        """The Fit-Hi-C p- and q-values of the map the triples define over bins 0 .. map_bins - 1
        (`ContactMap.significance`; docs/SPEC.md 2.9), bit for bit what `ContactMap.from_triples(
        ...).significance(...)` gives, without that matrix; `biases` and `q_max` go on to
        `FitHiC.fit_transform`.  One chromosome."""
        from .fithic import _significance      # (late: fithic takes this very type -- a real cycle)
        return _significance(self, int(map_bins), kwargs)

    def _graph_arguments(self, n_nodes, kind, alpha, KRnorm, KRexpected):
        """(n_nodes, kind code, alpha, KR pointers) of the graph calls, checked."""
        n = int(n_nodes)
        if n < 1:
            raise ValueError("n_nodes must be at least 1")
        if kind not in _KINDS:
            raise ValueError("kind must be 'counts' or 'wish'")
        if not float(alpha) > 0:
            raise ValueError("alpha must be positive")
        kr, ke = _kr_pair(KRnorm, KRexpected, n)
        return n, _KINDS[kind], float(alpha), kr, ke

    def edge_degrees(self, n_nodes, kind="counts", alpha=3.0, KRnorm=None, KRexpected=None):
        """The number of graph edges of every node 0 .. n_nodes - 1 (`bb_triples_edge_degrees`,
        docs/SPEC.md 2.1.2): the stored off-diagonal cells whose wish distance -- under `kind`,
        `alpha` and the KR vectors, as `fit_triples` forms it -- is finite and positive.  int64."""
        n, kind, alpha, kr, ke = self._graph_arguments(n_nodes, kind, alpha, KRnorm, KRexpected)
        deg = numpy.zeros(n, dtype=numpy.int64)
        self._call("edge_degrees", n, kind, alpha, kr, ke, deg.ctypes.data_as(_lib.p_i64))
        return deg

    def shortest_paths(self, n_nodes, sources, kind="counts", alpha=3.0, KRnorm=None, KRexpected=None):
        """The shortest-path lengths from the nodes `sources` (any order, repeats allowed, at most
        `GeodesicRows.MAX_SOURCES`) to all n_nodes nodes of the graph whose edges are the triples'
        wish distances (`bb_triples_paths`, docs/SPEC.md 2.1.2), without the dense matrix: a
        `GeodesicRows`, resident on the device.  Bit for bit scipy's Dijkstra in float64."""
        n, kind, alpha, kr, ke = self._graph_arguments(n_nodes, kind, alpha, KRnorm, KRexpected)
        src = numpy.ascontiguousarray(sources, dtype=numpy.int64).ravel()
        h = _lib.c_void_p()
        self._call("paths", n, kind, alpha, kr, ke, src.ctypes.data_as(_lib.p_i64), src.shape[0], h)
        return GeodesicRows(h)


class GeodesicRows(_lib.Handle):
    """What `DeviceTriples.shortest_paths` returns: the (n_sources, n_nodes) float64 geodesics,
    resident on the device as a `bb_paths`, which owns its memory (it may outlive the triples).
    `sweeps_`: Bellman-Ford sweeps made (not reproducible: the distances are updated in place);
    `unreachable_`: (source, node) pairs without a path.  A context manager; `close()` frees it,
    any other call after that is a ValueError."""
    MAX_SOURCES = 1024                      # BB_PATHS_MAX_SOURCES
    prefix = "bb_paths_"

    def __init__(self, handle):
        _lib.Handle.__init__(self, handle)
        ns, nn, sw, un = _lib.c_i64(), _lib.c_i64(), _lib.c_i64(), _lib.c_i64()
        self._call("info", ns, nn, sw, un)
        self.n_sources, self.n_nodes = int(ns.value), int(nn.value)
        self.sweeps_, self.unreachable_ = int(sw.value), int(un.value)

    def to_host(self):
        """(n_sources, n_nodes): 0 where no path exists and on a source's own node."""
        out = numpy.empty((self.n_sources, self.n_nodes), dtype=numpy.float64)
        self._call("read", _lib.as_f64_ptr(out))
        return out

    def columns(self, nodes):
        """(n_sources, len(nodes)): the distances to the listed nodes alone."""
        idx = numpy.ascontiguousarray(nodes, dtype=numpy.int64).ravel()
        out = numpy.empty((self.n_sources, idx.shape[0]), dtype=numpy.float64)
        self._call("read_columns", idx.ctypes.data_as(_lib.p_i64), idx.shape[0], _lib.as_f64_ptr(out))
        return out

    def reached(self):
        """int64 (n_sources,): the nodes every source has a path to, its own included."""
        out = numpy.zeros(self.n_sources, dtype=numpy.int64)
        self._call("reached", out.ctypes.data_as(_lib.p_i64))
        return out

    def place(self, coef, mu, out=None):
        """Landmark placement on the device (`bb_paths_place`): (xyz, placed).  xyz[j] =
        -1/2 sum_a coef[a] (D[j][a]^2 - mu[a]) for every node with a path from every source that
        takes part (a source whose coef row and mu are 0 does not); the other rows keep what
        `out` -- (n_nodes, 3) float64, C-ordered; None: zeros -- held.  placed: bool."""
        coef = numpy.ascontiguousarray(coef, dtype=numpy.float64)
        mu = numpy.ascontiguousarray(mu, dtype=numpy.float64)
        if coef.shape != (self.n_sources, 3) or mu.shape != (self.n_sources,):
            raise ValueError("coef must have shape (n_sources, 3) and mu (n_sources,)")
        if out is None:
            out = numpy.zeros((self.n_nodes, 3), dtype=numpy.float64)
        if (not isinstance(out, numpy.ndarray) or out.dtype != numpy.float64
                or out.shape != (self.n_nodes, 3) or not out.flags.c_contiguous):
            raise ValueError("out must be a C-ordered float64 array of shape (n_nodes, 3)")
        placed = numpy.zeros(self.n_nodes, dtype=numpy.uint8)
        self._call("place", _lib.as_f64_ptr(coef), _lib.as_f64_ptr(mu), _lib.as_f64_ptr(out),
                   placed.ctypes.data_as(_lib.p_u8))
        return out, placed.astype(bool)

    def timing(self):
        """(weights_ms, sweeps_ms) of the call that made these rows, by HIP events."""
        w, s = _lib.c_dbl(), _lib.c_dbl()
        self._call("timing", w, s)
        return float(w.value), float(s.value)


def _check_triples(triples):
    """The float64 (n, 3) view of `triples`, or ValueError."""
    return triples_buffer(triples)[0]


def _bin_count(n_bins):
    n = int(n_bins)
    if n < 0:
        raise ValueError("n_bins must not be negative")
    return n


@contextlib.contextmanager
def _resident_triples(triples, resolution, devices):
    """The `DeviceTriples` a call works on.  A caller's own is yielded as it is and stays open;
    anything else is uploaded -- once per distinct device of `devices`, the copy on devices[0]
    being the one yielded and, where there are several entries, naming them all as its
    `per_device` (what `GroupEngine.set_wish_triples` reads) -- and closed on exit."""
    if isinstance(triples, DeviceTriples):
        yield triples
        return
    if int(resolution) <= 0:
        raise ValueError("resolution must be positive")
    per_device = {}
    try:
        for d in devices:
            if d not in per_device:
                per_device[d] = DeviceTriples(triples, resolution, d)
        dev = per_device[devices[0]]
        if len(devices) > 1:
            dev.per_device = per_device
        yield dev
    finally:
        for t in per_device.values():
            t.close()


_BALANCE_KEYS = ("ignore_diags", "min_nnz", "tol", "max_iter", "row_sum")


def _balance_options(balance):
    """`fit_triples(balance=...)` as (checked keyword arguments of `DeviceTriples.balance`, whether
    the expected is wanted), without touching the library."""
    if balance is True:
        balance = {}
    if not isinstance(balance, dict):
        raise ValueError("balance must be None, True or a dict of balance_triples' arguments")
    unknown = sorted(set(balance) - set(_BALANCE_KEYS) - {"expected"})
    if unknown:
        raise ValueError("balance: unknown argument %r" % (unknown[0],))
    args = {k: balance[k] for k in _BALANCE_KEYS if k in balance}
    return dict(zip(_BALANCE_KEYS, check_balance_args(**args))), bool(balance.get("expected", False))


class TriplesBalance(object):
    """What `balance_triples` returns: `bias` (length n_bins, NaN at masked bins), `masked` (bool),
    `iterations`, `variance`, `converged`; `expected`, `expected_sums`, `expected_counts` (None
    unless asked for)."""

    def __init__(self, dev, bias, expected=None):
        self.bias, self.masked = bias, dev.balance_masked_
        self.iterations, self.variance = dev.balance_iterations_, dev.balance_variance_
        self.converged = dev.balance_converged_
        self.expected = expected
        self.expected_sums = None if expected is None else dev.expected_sums_
        self.expected_counts = None if expected is None else dev.expected_counts_


def balance_triples(triples, resolution, n_bins, ignore_diags=0, min_nnz=0, tol=1e-5, max_iter=200,
                    row_sum=None, expected=False, device=None):
    """Balance a raw map straight from its Rao-format (n, 3) triples [pos_i, pos_j, count],
    never building the dense matrix (docs/SPEC.md 2.5.3): the ICE bias vector -- and with
    expected=True the distance-decay expected of the balanced map -- that
    `ContactMap.from_triples(triples, resolution, n_bins)` followed by `balance(...)` and
    `expected()` defines.  Returns a `TriplesBalance`.  `triples` may be a `DeviceTriples`
    (its own resolution and device are used; it stays open)."""
    args = dict(zip(_BALANCE_KEYS, check_balance_args(ignore_diags, min_nnz, tol, max_iter, row_sum)))
    n = _bin_count(n_bins)
    with _resident_triples(triples, resolution, [pick_device(device, several_ranks())]) as dev:
        bias = dev.balance(n, **args)
        return TriplesBalance(dev, bias, dev.expected(n, bias) if expected else None)


def coarsen_triples(triples, resolution, n_bins, factor, how="sum", device=None):
    """Pool a map straight from its Rao-format (n, 3) triples [pos_i, pos_j, count], never
    building the dense matrix (`DeviceTriples.coarsen`; docs/SPEC.md 2.12), host to host: returns
    (pooled, nc) -- the (m, 3) float64 triples at resolution `resolution * factor`, in canonical
    order, and nc = ceil(n_bins / factor).  `ContactMap.from_triples(pooled, resolution * factor,
    nc)` is bit for bit `ContactMap.from_triples(triples, resolution, n_bins).coarsen(factor,
    how)`.  `triples` may be a `DeviceTriples` (its own resolution and device are used; it stays
    open)."""
    check_coarsen_args(factor, how)
    n = _bin_count(n_bins)
    with _resident_triples(triples, resolution, [pick_device(device, several_ranks())]) as dev:
        with dev.coarsen(n, factor, how) as pooled:
            return pooled.to_host(), pooled.n_bins_


def insulation_triples(triples, resolution, n_bins, window, ignore_diags=2, bias=None, min_valid=0.66,
                       device=None):
    """The insulation score and the domain boundaries of a map straight from its Rao-format (n, 3)
    triples [pos_i, pos_j, count], never building the dense matrix (`DeviceTriples.insulation`;
    docs/SPEC.md 2.13): the `InsulationTrack` that `ContactMap.from_triples(triples, resolution,
    n_bins).insulation(window, ignore_diags, bias, min_valid)` gives, bit for bit.  `triples` may
    be a `DeviceTriples` (its own resolution and device are used; it stays open)."""
    check_insulation_args(window, ignore_diags, min_valid)
    n = _bin_count(n_bins)
    with _resident_triples(triples, resolution, [pick_device(device, several_ranks())]) as dev:
        return dev.insulation(n, window, ignore_diags, bias, min_valid)
