"""StructureSolver -- contact matrix -> 3D coordinates on MI355X.

Host side of the hot path BASELINE.json names.  The reference has no solver
(SURVEY.md section 0); the estimator shape follows the only estimator the
reference has, `FitHiC(hyper-parameters).fit_transform(data)`
(`blueberry/fithic.py:76-108`), and the input is the dense float64 matrix a
`ContactMap` holds (`blueberry/datatypes.pyx:78-86`).  The algorithm is
specified in docs/SPEC.md and runs entirely in libblueberry_hip.so
(include/blueberry_hip.h); this module only validates arguments, owns the
handle and, for world_size > 1, drives one all-reduce per iteration through
torch.distributed (backend "nccl" = RCCL over xGMI) -- or, with
`StructureSolver(devices=[...])`, drives several GPUs from this one process without
torch (`GroupEngine`: one solver per device, one host thread each, the sum over them
ordered by HIP events, `bb_group_*`).
"""
import contextlib
import math
import os
import sys

import numpy

from . import _lib
from .datatypes import (_balance, _expected, _nan_to_num, _pick_device, check_balance_args,
                        check_coarsen_args, triples_buffer)

_DTYPES = {"float32": _lib.BB_F32, "float64": _lib.BB_F64}
_KINDS = {"wish": _lib.BB_KIND_WISH, "counts": _lib.BB_KIND_COUNTS}


class RankDeficient(RuntimeError):
    """The block power iteration of the device-resident spectral start lost rank: the map has
    fewer than three independent directions (an empty or unconstrained map, fewer than 4 bins).
    `fit()` then takes the host-driven start; every other library error propagates."""


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

    def significance(self, map_bins, **kwargs):
        """The Fit-Hi-C p- and q-values of the map the triples define over bins 0 .. map_bins - 1
        (`ContactMap.significance`; docs/SPEC.md 2.9), bit for bit what `ContactMap.from_triples(
        ...).significance(...)` gives, without that matrix; `biases` and `q_max` go on to
        `FitHiC.fit_transform`.  One chromosome."""
        from .fithic import _significance
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


def landmark_choice(live, n_landmarks):
    """The landmarks of docs/SPEC.md 2.5.4 among the live nodes `live` (ascending):
    L = min(n_landmarks, len(live)) of them, landmark k = live[((2 k + 1) len(live)) // (2 L)]."""
    live = numpy.asarray(live, dtype=numpy.int64)
    L = min(int(n_landmarks), live.shape[0])
    k = numpy.arange(L, dtype=numpy.int64)
    return live[((2 * k + 1) * live.shape[0]) // (2 * max(L, 1))]


def landmark_coefficients(G_LL):
    """(coef, mu) of landmark MDS (de Silva & Tenenbaum) from the (L, L) geodesics among the
    landmarks, docs/SPEC.md 2.5.4 -- the only place the rule lives; pure numpy.
    Delta2 = (G^2 + G^2.T) / 2, mu = its column means, B = -J Delta2 J / 2, numpy.linalg.eigh,
    the three largest eigenvalues l_c with their vectors v_c, each vector's sign such that its
    entry of largest magnitude (lowest index on ties) is positive; coef[:, c] = v_c / sqrt(l_c),
    a zero column where l_c <= 1e-12 l_1 (a flat or collinear map).  A node with squared
    geodesics d2 to the landmarks is placed at -coef.T (d2 - mu) / 2."""
    G = numpy.asarray(G_LL, dtype=numpy.float64)
    if G.ndim != 2 or G.shape[0] != G.shape[1] or G.shape[0] < 1:
        raise ValueError("G_LL must be a square (L, L) array")
    L = G.shape[0]
    sq = G * G
    d2 = 0.5 * (sq + sq.T)
    mu = d2.mean(axis=0)
    J = numpy.eye(L) - 1.0 / L
    B = -0.5 * (J @ d2 @ J)
    w, V = numpy.linalg.eigh(B)
    order = numpy.argsort(w, kind="stable")[::-1][:3]
    coef = numpy.zeros((L, 3))
    top = w[order[0]]
    for c, q in enumerate(order):
        if top > 0.0 and w[q] > 1e-12 * top:
            v = V[:, q]
            if v[numpy.argmax(numpy.abs(v))] < 0.0:
                v = -v
            coef[:, c] = v / numpy.sqrt(w[q])
    return coef, mu


class LandmarkInfo(object):
    """What `landmark_start(..., return_info=True)` tells besides the start: `landmarks_` (the L
    landmark nodes), `kept_` (bool per landmark: reached by the main one), `placed_` (bool per
    node), `sweeps_` and `unreachable_` of the shortest paths; with keep_rows=True `rows_`, the
    open `GeodesicRows` of the landmarks (the caller closes them), else None."""

    def __init__(self, landmarks, kept, placed, sweeps, unreachable, rows=None):
        self.landmarks_, self.kept_, self.placed_ = landmarks, kept, placed
        self.sweeps_, self.unreachable_ = sweeps, unreachable
        self.rows_ = rows


def _check_n_landmarks(n_landmarks):
    if (isinstance(n_landmarks, bool) or not isinstance(n_landmarks, (int, numpy.integer))
            or not 4 <= int(n_landmarks) <= GeodesicRows.MAX_SOURCES):
        raise ValueError("n_landmarks must be an int in [4, %d]" % GeodesicRows.MAX_SOURCES)
    return int(n_landmarks)


def _check_landmark_weight(weight):
    if (isinstance(weight, bool) or not isinstance(weight, (int, float, numpy.integer, numpy.floating))
            or not numpy.isfinite(weight) or weight < 0):
        raise ValueError("landmark_weight must be a finite number >= 0")
    return float(weight)


def landmark_start(triples, resolution, n_bins, n_landmarks=64, kind="counts", alpha=3.0, KRnorm=None,
                   KRexpected=None, seed=0, device=0, return_info=False, keep_rows=False):
    """A start for sparse maps that holds the global fold (docs/SPEC.md 2.5.4): landmark MDS
    (L-Isomap) over the graph of the triples' wish distances, never forming the dense matrix.
    Landmarks are spread evenly over the bins that have an edge; shortest paths run from them on
    the device (`DeviceTriples.shortest_paths`); the landmark that reaches the most nodes (the
    lowest on ties) is the main one, landmarks it does not reach are dropped (fewer than 4 left:
    ValueError); `landmark_coefficients` of the kept landmarks' mutual geodesics place every node
    the main landmark reaches, on the device (the (L, N) array never travels to the host).  Nodes
    that are not placed -- dead bins, small components -- keep the rows of the seeded default start
    `numpy.random.default_rng(seed).standard_normal((n_bins + 1, 3))`.
    Returns the (n_bins + 1, 3) float64 array; with return_info=True, (array, `LandmarkInfo`).
    keep_rows=True (with return_info) leaves the geodesic rows open as `info.rows_` -- what
    `HipEngine.set_anchors` copies for a fit with landmark constraints (SPEC 2.5.5).
    `triples` may be a `DeviceTriples` (its own resolution and device are used; it stays open)."""
    n_landmarks = _check_n_landmarks(n_landmarks)
    n = _bin_count(n_bins) + 1
    graph = dict(kind=kind, alpha=alpha, KRnorm=KRnorm, KRexpected=KRexpected)
    with _resident_triples(triples, resolution, [_pick_device(device)]) as dev:
        live = numpy.flatnonzero(dev.edge_degrees(n, **graph) > 0)
        landmarks = landmark_choice(live, n_landmarks)
        few = "the map is too disconnected for a landmark start: %s (need 4)"
        if landmarks.shape[0] < 4:
            raise ValueError(few % ("%d bins have an edge" % live.shape[0]))
        rows = dev.shortest_paths(n, landmarks, **graph)
        try:
            main = int(numpy.argmax(rows.reached()))           # (the lowest index on ties)
            G = rows.columns(landmarks)
            kept = G[main] > 0.0
            kept[main] = True
            if int(kept.sum()) < 4:
                raise ValueError(few % ("%d landmarks lie in the largest component" % int(kept.sum())))
            coef, mu = numpy.zeros((landmarks.shape[0], 3)), numpy.zeros(landmarks.shape[0])
            coef[kept], mu[kept] = landmark_coefficients(G[numpy.ix_(kept, kept)])
            start = numpy.random.default_rng(int(seed)).standard_normal((n, 3))
            start, placed = rows.place(coef, mu, out=start)
            keep = bool(keep_rows and return_info)
            info = LandmarkInfo(landmarks, kept, placed, rows.sweeps_, rows.unreachable_,
                                rows if keep else None)
            if keep:
                rows = None
        finally:
            if rows is not None:
                rows.close()
    return (start, info) if return_info else start


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
    with _resident_triples(triples, resolution, [_pick_device(device)]) as dev:
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
    with _resident_triples(triples, resolution, [_pick_device(device)]) as dev:
        with dev.coarsen(n, factor, how) as pooled:
            return pooled.to_host(), pooled.n_bins_


class HipEngine(_lib.Handle):
    """One rank's device state: thin, 1:1 over the bb_solver_* C-ABI."""

    prefix = "bb_solver_"
    n_maps = 1                      # several once set_maps() has laid them end to end

    def __init__(self, n_bins, dtype, rank=0, world=1, device=0, tiles=None):
        _lib.Handle.__init__(self)
        self.n_bins, self.dtype, self.rank, self.world, self.device = (
            int(n_bins), dtype, int(rank), int(world), int(device))
        if tiles is None:
            ti = tj = None
            nt = 0
        else:
            ti = numpy.ascontiguousarray(tiles[0], dtype=numpy.int32)
            tj = numpy.ascontiguousarray(tiles[1], dtype=numpy.int32)
            if ti.shape != tj.shape or ti.ndim != 1:
                raise ValueError("tiles must be a pair of equal-length 1-D index arrays")
            nt = ti.shape[0]
        self._create(self.n_bins, _DTYPES[dtype], self.device, self.rank, self.world,
                     None if ti is None else ti.ctypes.data_as(_lib.p_i32),
                     None if tj is None else tj.ctypes.data_as(_lib.p_i32), nt)
        self._exch = None
        self._comm_state = None     # "peer" | "rccl" | "torch" | "host" once chosen
        self._peer = None           # outcome of peer_setup()
        self._peer_error = ""
        self._comm_trial = None     # timings of select_exchange's trial, if one ran
        self._comm_trial_error = None   # what made a leg of that trial fail on this rank

    # -- lifetime ---------------------------------------------------------
    def close(self):
        _lib.Handle.close(self)
        self._exch = None

    # -- layout -----------------------------------------------------------
    def layout(self):
        info = _lib.LayoutInfo()
        ub, ue = _lib.c_i64(), _lib.c_i64()
        self._call("layout", info, ub, ue)
        d = info.as_dict()
        d["u_begin"], d["u_end"] = int(ub.value), int(ue.value)
        return d

    # -- inputs -----------------------------------------------------------
    def set_wish_dense(self, matrix, kind, alpha):
        m = _check_square(matrix, self.n_bins)
        self._call("set_wish_dense", _lib.as_f64_ptr(m), m.strides[0] // 8, _KINDS[kind],
                   float(alpha))

    def set_wish_from_cm(self, dev_matrix, kind, alpha):
        """Device to device from a resident ContactMap matrix (datatypes._DeviceMatrix)."""
        self._call("set_wish_from_cm", dev_matrix._open(), _KINDS[kind], float(alpha))

    def set_wish_resident(self, cm, kind, alpha):
        """A resident ContactMap: device to device when it lives on this engine's GPU."""
        dev = cm._resident()
        if dev.device == self.device:
            self.set_wish_from_cm(dev, kind, alpha)
        else:
            # the map lives on another GPU than this rank's solver (a ContactMap made with
            # an explicit device): through the host once, like a plain matrix
            self.set_wish_dense(cm.to_host(), kind, alpha)

    def set_wish_sparse(self, rows, cols, vals, kind, alpha, KRnorm=None, KRexpected=None):
        r = numpy.ascontiguousarray(rows, dtype=numpy.int64)
        c = numpy.ascontiguousarray(cols, dtype=numpy.int64)
        v = numpy.ascontiguousarray(vals, dtype=numpy.float64)
        if not (r.ndim == c.ndim == v.ndim == 1 and r.shape == c.shape == v.shape):
            raise ValueError("rows, cols, vals must be 1-D arrays of equal length")
        kr, ke = _kr_pair(KRnorm, KRexpected, self.n_bins)
        self._call("set_wish_sparse", r.ctypes.data_as(_lib.p_i64), c.ctypes.data_as(_lib.p_i64),
                   _lib.as_f64_ptr(v), r.shape[0], _KINDS[kind], float(alpha), kr, ke)

    def set_wish_triples(self, dev_triples, kind, alpha, KRnorm=None, KRexpected=None):
        """From triples resident on the device (`DeviceTriples`): binned, KR / O-E
        normalised and converted there."""
        kr, ke = _kr_pair(KRnorm, KRexpected, self.n_bins)
        self._call("set_wish_triples", dev_triples._open(), _KINDS[kind], float(alpha), kr, ke)

    # -- several maps in one solver (bb_solver_set_maps) -----------------------
    def set_maps(self, bin_begin, lr_scale):
        """Declare the maps laid end to end in this solver: map m owns the bins
        [bin_begin[m], bin_begin[m + 1]) and steps with lr * lr_scale[m]."""
        b = numpy.ascontiguousarray(bin_begin, dtype=numpy.int64)
        sc = numpy.ascontiguousarray(lr_scale, dtype=numpy.float64)
        if b.ndim != 1 or sc.ndim != 1 or b.shape[0] != sc.shape[0] + 1:
            raise ValueError("bin_begin needs one entry more than lr_scale")
        self._call("set_maps", sc.shape[0], b.ctypes.data_as(_lib.p_i64), _lib.as_f64_ptr(sc))
        self.n_maps = int(sc.shape[0])

    def set_wish_dense_block(self, matrix, bin_offset, kind, alpha):
        m = _check_square(matrix, numpy.asarray(matrix).shape[0])
        self._call("set_wish_dense_block", _lib.as_f64_ptr(m), m.strides[0] // 8, m.shape[0],
                   int(bin_offset), _KINDS[kind], float(alpha))

    def set_wish_from_cm_block(self, dev_matrix, bin_offset, kind, alpha):
        self._call("set_wish_from_cm_block", dev_matrix._open(), int(bin_offset), _KINDS[kind],
                   float(alpha))

    def _set_steps(self, name, scale, per):
        if scale is None:
            self._call(name, None, 0)
            return
        sc = numpy.ascontiguousarray(scale, dtype=numpy.float64)
        if sc.ndim != 1:
            raise ValueError("scale must be one factor per " + per)
        self._call(name, _lib.as_f64_ptr(sc), sc.shape[0])

    def set_block_steps(self, scale):
        """A step per block of the layout (`bb_solver_set_block_steps`): bin i moves by
        lr * scale[i // vw] * g_i; None = one step for all again."""
        self._set_steps("set_block_steps", scale, "block")

    def set_bin_steps(self, scale):
        """A step per bin (`bb_solver_set_bin_steps`): bin i moves by lr * scale[i] * g_i;
        None = one step for all again."""
        self._set_steps("set_bin_steps", scale, "bin")

    def degrees(self):
        """Per bin, the number of this rank's stored pairs that constrain it (delta > 0):
        `bb_solver_degrees`, one pass over the resident units."""
        out = numpy.zeros(self.n_bins, dtype=numpy.int64)
        self._call("degrees", out.ctypes.data_as(_lib.p_i64), out.shape[0])
        return out

    def set_weight_power(self, q):
        """Weighted stress (SPEC 2.3.1): w = delta^-q, q in {0, 1, 2}
        (`bb_solver_set_weight_power`)."""
        self._call("set_weight_power", int(q))

    def weight_sums(self):
        """Per bin, s_i = sum_j delta_ij^-q over this rank's stored pairs, float64
        (`bb_solver_weight_sums`; q = 0: the degrees)."""
        out = numpy.zeros(self.n_bins, dtype=numpy.float64)
        self._call("weight_sums", _lib.as_f64_ptr(out), out.shape[0])
        return out

    anchored = False                # landmark constraints resident (set_anchors)

    def set_anchors(self, rows, kept=None, weight=0.0):
        """Landmark constraints inside the fit (SPEC 2.5.5, `bb_solver_set_anchors`): the engine
        makes its own copy of the rows of `rows` (a `GeodesicRows`) with kept[a] true (None:
        all), which may be closed afterwards.  rows None or weight 0 clears them."""
        k = None
        if rows is not None and kept is not None:
            k = numpy.ascontiguousarray(kept, dtype=numpy.uint8)
            if k.shape != (rows.n_sources,):
                raise ValueError("kept must have one entry per source")
        self._call("set_anchors", None if rows is None else rows._open(),
                   None if k is None else k.ctypes.data_as(_lib.p_u8), float(weight))
        self.anchored = self.anchor_info()[0] > 0

    def anchor_sums(self):
        """Per bin, weight * sum of D^-q over the landmark terms that touch it, float64
        (`bb_solver_anchor_sums`): what joins `weight_sums` in the steps of SPEC 2.4.1."""
        out = numpy.zeros(self.n_bins, dtype=numpy.float64)
        self._call("anchor_sums", _lib.as_f64_ptr(out), out.shape[0])
        return out

    def anchor_stress(self):
        """The landmark terms' share of the stress at the current coordinates."""
        return float(self._get(_lib.c_dbl, "anchor_stress"))

    def anchor_info(self):
        """(kept rows, terms, bytes resident) of the anchors; zeros without."""
        rows, terms, nbytes = _lib.c_i64(), _lib.c_i64(), _lib.c_i64()
        self._call("anchor_info", rows, terms, nbytes)
        return int(rows.value), int(terms.value), int(nbytes.value)

    def score(self, xyz=None):
        """The sums of SPEC 2.8 over this rank's units (`bb_solver_score`): (profile, bins),
        float64 of shape (n_bins, 9) and (n_bins, 3).  xyz: the structure to score; None: the
        engine's own coordinates."""
        profile = numpy.zeros((self.n_bins, 9), dtype=numpy.float64)
        bins = numpy.zeros((self.n_bins, 3), dtype=numpy.float64)
        self._call("score", None if xyz is None else _lib.as_f64_ptr(_check_coords(xyz, self.n_bins)),
                   _lib.as_f64_ptr(profile), _lib.as_f64_ptr(bins))
        return profile, bins

    def loglog(self, xyz=None):
        """The log-log sums of SPEC 2.11 over this rank's units (`bb_solver_loglog`): float64 of
        shape (n_bins, 7), row k = the pairs of separation k: pairs with d > 0, sum u, sum v,
        sum u^2, sum v^2, sum u v (u = log delta, v = log d), pairs with d = 0.  xyz as `score`."""
        profile = numpy.zeros((self.n_bins, 7), dtype=numpy.float64)
        self._call("loglog", None if xyz is None else _lib.as_f64_ptr(_check_coords(xyz, self.n_bins)),
                   _lib.as_f64_ptr(profile))
        return profile

    def repower(self, p):
        """Every stored wish distance w > 0 becomes w^p under the wish rule of SPEC 2.1, in place
        (`bb_solver_repower`); degrees and weight sums are the caller's to recompute."""
        self._call("repower", float(p))

    def stress_maps(self):
        out = numpy.empty(self.n_maps, dtype=numpy.float64)
        self._call("stress_maps", _lib.as_f64_ptr(out), out.shape[0])
        return out

    def set_wish_from_coords(self, xstar):
        self._call("set_wish_from_coords", _lib.as_f64_ptr(_check_coords(xstar, self.n_bins)))

    def set_coords(self, x0):
        self._call("set_coords", _lib.as_f64_ptr(_check_coords(x0, self.n_bins)))

    def get_coords(self):
        out = numpy.empty((self.n_bins, 3), dtype=numpy.float64)
        self._call("get_coords", _lib.as_f64_ptr(out))
        return out

    # -- iterations -------------------------------------------------------
    def set_momentum(self, mu):
        self._call("set_momentum", float(mu))

    def iterate(self, iters, lr):
        self._call("iterate", int(iters), float(lr))

    def grad(self):
        self._call("grad")

    def apply(self, lr):
        self._call("apply", float(lr))

    def matvec_sq(self, x):
        """(D o D) @ x for this rank's units; x is (n_bins, 3)."""
        x = _check_coords(x, self.n_bins)
        y = numpy.empty_like(x)
        self._call("matvec_sq", _lib.as_f64_ptr(x), _lib.as_f64_ptr(y))
        return y

    def spectral_init_device(self, n_iter, v0, tol=0.0):
        """Classical-MDS start computed and left on the device: `bb_solver_spectral_init_tol`.
        v0: (n_bins, 3) start of the block power iteration (the same on every rank).  With
        several ranks it is collective and needs their exchange set up first (peer arenas or
        the library's communicator): the per-rank products are summed on the device, nothing
        of size N crosses PCIe.  tol > 0: n_iter is the most products made; the loop ends once
        B V lies within tol (relative) of span(V).  Returns (products orthonormalised, last
        distance read or -1).  Raises RankDeficient when the iterate lost rank."""
        v0 = _check_coords(v0, self.n_bins)
        done, res = _lib.c_int(), _lib.c_dbl()
        # explicit: a lost rank is an outcome of its own (the caller takes the host-driven start)
        rc = self._status("spectral_init_tol", int(n_iter), float(tol), _lib.as_f64_ptr(v0), done, res)
        if rc == _lib.BB_ERR_STATE and "lost rank" in _lib.last_error():
            raise RankDeficient(_lib.last_error())
        _lib.check(rc, "bb_solver_spectral_init_tol")
        return int(done.value), float(res.value)

    def stress(self):
        return float(self._get(_lib.c_dbl, "stress"))

    def stress_history(self):
        out = numpy.empty(int(self._get(_lib.c_i64, "get_stress_history", None, 0)),
                          dtype=numpy.float64)
        if out.size:
            self._get(_lib.c_i64, "get_stress_history", _lib.as_f64_ptr(out), out.size)
        return out

    def sync(self):
        self._call("sync")

    def exchange_size(self):
        return int(self._get(_lib.c_i64, "exchange_size"))

    def read_exchange(self):
        """Exchange buffer [g (n_pad,3) | stress hi | lo] as float64 on the host."""
        out = numpy.empty(self.exchange_size(), dtype=numpy.float64)
        self._call("read_exchange", _lib.as_f64_ptr(out), out.size)
        return out

    def write_exchange(self, host):
        host = numpy.ascontiguousarray(host, dtype=numpy.float64)
        self._call("write_exchange", _lib.as_f64_ptr(host), host.size)

    # -- the all-reduce boundary (world > 1) --------------------------------
    def comm_setup(self):
        """Make the library's own RCCL communicator for this job: rank 0 draws the
        128-byte id, torch.distributed only carries it to the other ranks, every
        rank joins (`ncclCommInitRank`).  Collective.  Returns False -- on every
        rank alike -- when RCCL cannot be used, so that the caller can fall back
        to the torch.distributed all-reduce."""
        import ctypes
        import torch.distributed as dist
        box = [None]
        if self.rank == 0:
            buf = ctypes.create_string_buffer(128)
            if self._lib.bb_comm_unique_id(buf) == _lib.BB_OK:
                box[0] = buf.raw
        dist.broadcast_object_list(box, src=0)
        if box[0] is None:
            return False
        # explicit: a failure here is this rank's vote, not an error
        ok = self._status("comm_init", box[0]) == _lib.BB_OK
        # all ranks must take the same path: agree on the outcome
        import torch
        flag = torch.tensor([1 if ok else 0], dtype=torch.int32,
                            device=torch.device("cuda", self.device))
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        return bool(flag.item())

    # the library's communicator cache (bb_comm_cached / bb_solver_comm_attach / _detach):
    # `comm_reuse` below drives these three
    def _comm_cached(self):
        import ctypes
        have = ctypes.c_int(0)
        self._lib.bb_comm_cached(self.device, self.rank, self.world, ctypes.byref(have))
        return bool(have.value)

    def _comm_generation(self):
        """Generation of the free cached communicator for this engine's key -- a hash of the
        unique id it was made with, equal on the ranks that made it together -- or 0."""
        import ctypes
        have, gen = ctypes.c_int(0), ctypes.c_uint64(0)
        self._lib.bb_comm_cached_generation(self.device, self.rank, self.world,
                                            ctypes.byref(have), ctypes.byref(gen))
        return int(gen.value) if have.value else 0

    def _comm_attach(self):
        # explicit: the outcome is agreed between the ranks (`comm_reuse`), not raised
        return self._status("comm_attach") == _lib.BB_OK

    def _comm_detach(self):
        self._status("comm_detach")

    def iterate_dist(self, iters, lr):
        """`iters` x { grad, RCCL all-reduce, apply }, all enqueued by one C call."""
        self._call("iterate_dist", int(iters), float(lr))

    def peer_setup(self):
        """Connect the peer exchange (one-shot all-reduce inside the solver's own
        kernels, include/blueberry_hip.h): every rank exports its receive arena,
        torch.distributed only carries the 128-byte handles, every rank maps all
        arenas.  Collective.  Returns False -- on every rank alike -- when any
        rank could not export or map, so that the caller can fall back to RCCL."""
        import ctypes
        import torch.distributed as dist
        if self._peer is not None:
            return self._peer
        buf = ctypes.create_string_buffer(_lib.BB_PEER_HANDLE_BYTES)
        # explicit, here and at the connect: a failure is this rank's vote, not an error
        mine = buf.raw if self._status("peer_export", buf) == _lib.BB_OK else None
        handles = [None] * self.world
        dist.all_gather_object(handles, mine)
        ok = all(h is not None for h in handles)
        if ok:
            ok = self._status("peer_connect", b"".join(handles)) == _lib.BB_OK
        if not ok:
            self._peer_error = _lib.last_error()
        oks = [None] * self.world
        dist.all_gather_object(oks, bool(ok))
        self._peer = all(oks)
        return self._peer

    def iterate_peer(self, iters, lr):
        """`iters` x { grad, reduce + push to every peer, wait + rank-ordered sum +
        update }, all enqueued by one C call."""
        self._call("iterate_peer", int(iters), float(lr))

    def sync_timeout(self, milliseconds):
        """sync() that raises RuntimeError if the stream has not drained in time."""
        self._call("sync_timeout", int(milliseconds))

    def comm_abort(self):
        self._call("comm_abort")

    def peer_form(self):
        """'one launch' (reduce, push, wait, sum and update in one kernel) or 'two launches'
        (include/blueberry_hip.h, peer exchange)."""
        return "one launch" if self._get(_lib.c_int, "peer_form") else "two launches"

    def peer_set_form(self, one_launch):
        """Choose the exchange's form before its first use (the same on every rank)."""
        self._call("peer_set_form", 1 if one_launch else 0)

    def peer_set_timeout(self, milliseconds):
        self._call("peer_set_timeout", int(milliseconds))

    def comm_world(self):
        """Ranks RCCL reports for the library's communicator, or None without one."""
        n = _lib.c_int()
        # explicit: no communicator is an answer (None), not an error
        if self._status("comm_world", n) != _lib.BB_OK:
            return None
        return int(n.value)

    def peer_status(self):
        """Synchronise and raise if a peer wait ran into its time limit."""
        return int(self._get(_lib.c_int, "peer_status"))

    def exchange_tensor(self):
        """A torch tensor aliasing the exchange buffer [g (n_pad,3) | hi | lo].

        torch allocates it (plumbing: it is what torch.distributed can reduce)
        and the solver is told to write its partial gradient there; the solver
        is also moved onto torch's current stream so that the collective and
        the kernels are ordered without host synchronisation."""
        if self._exch is None:
            import torch
            rts = _lib.hip_runtimes_loaded()
            if len(rts) > 1:
                raise RuntimeError(
                    "two HIP runtimes are loaded (%s): import torch BEFORE the first "
                    "blueberry_amd compute call in a distributed job, so that "
                    "libblueberry_hip.so binds to the runtime torch uses" % ", ".join(rts))
            tdt = torch.float32 if self.dtype == "float32" else torch.float64
            dev = torch.device("cuda", self.device)
            self._exch = torch.zeros(self.exchange_size(), dtype=tdt, device=dev)
            stream = torch.cuda.current_stream(dev)
            self._call("set_stream", _lib.c_void_p(stream.cuda_stream))
            self._call("set_exchange_buffer", _lib.c_void_p(self._exch.data_ptr()))
        return self._exch

    # -- measurement ------------------------------------------------------
    def set_timing(self, enabled):
        """True / 1: HIP events around every iteration; k > 1: every k-th; False: off."""
        self._call("set_timing", int(enabled))

    def timing(self):
        g, r, n = _lib.c_dbl(), _lib.c_dbl(), _lib.c_i64()
        self._call("get_timing", g, r, n)
        return {"grad_ms": float(g.value), "reduce_ms": float(r.value), "launches": int(n.value),
                "step_ms": float(self._get(_lib.c_dbl, "get_step_timing"))}

    def score_timing(self):
        """(profile_ms, fold_ms, bins_ms) of the last `score` or `loglog` (bins_ms = 0) made with
        timing on."""
        t = [_lib.c_dbl() for _ in range(3)]
        self._call("get_score_timing", *t)
        return tuple(float(v.value) for v in t)

    def event_gap_ms(self, pairs=16):
        """Average ms between two HIP events recorded back to back behind a sweep launch:
        what an event-timed interval contains besides its kernel (measurement aid)."""
        return float(self._get(_lib.c_dbl, "measure_event_gap", int(pairs)))

    def anchor_ms(self, launches=10):
        """Average ms of one iteration's three anchor launches alone (`bb_solver_measure_anchors`;
        measurement aid)."""
        return float(self._get(_lib.c_dbl, "measure_anchors", int(launches)))

    def stream_read_ms(self, launches=10):
        """Average ms of a read-only sweep over the resident units (measurement aid)."""
        return float(self._get(_lib.c_dbl, "measure_stream_read", int(launches)))

    def iteration_path(self):
        """'row_owner' (small one-rank maps: one launch per iteration) or 'units'."""
        ro, wpr = _lib.c_int(), _lib.c_int()
        self._call("iteration_path", ro, wpr)
        return ("row_owner", int(wpr.value)) if ro.value else ("units", 0)

    def traffic(self):
        b, p = _lib.c_i64(), _lib.c_i64()
        self._call("traffic", b, p)
        return {"unit_bytes": int(b.value), "pairs_dense": int(p.value)}

    def stream_info(self):
        """The 24-bit stream the fp32 stress sweep reads instead of the units, where it is in
        use (`bb_solver_stream_info`): units held packed and raw, its bytes and the changes of
        format between consecutive units; packed_units 0 and stream_bytes 0 with no stream."""
        v = [_lib.c_i64() for _ in range(4)]
        self._call("stream_info", *v)
        return dict(zip(("packed_units", "raw_units", "stream_bytes", "format_switches"),
                        (int(x.value) for x in v)))


class GroupEngine(_lib.Handle):
    """Several GPUs from ONE process (`bb_group_*`): member r is a HipEngine playing rank r of
    world R on devices[r] (a device may repeat: members then share it), each holding only its
    own units; one host thread per member enqueues its iterations, and the partials are summed
    by group_apply_kernel in rank order, ordered by HIP events.  To `StructureSolver` it looks
    like one engine of world 1: every setter goes to all members, degrees, weight sums, matvecs
    and scores come back summed over the members in rank order (float64 / int64), coordinates and
    stress history are member 0's -- all members hold the same bits."""
    prefix = "bb_group_"

    def __init__(self, n_bins, dtype, devices, tiles=None):
        _lib.Handle.__init__(self)
        self.n_bins, self.dtype = int(n_bins), dtype
        self.devices = [int(d) for d in devices]
        self.device = self.devices[0]
        self.world = 1                     # what the caller sees: one engine, summed results
        self._comm_state = "group"
        self.members = []
        try:
            R = len(self.devices)
            for r, d in enumerate(self.devices):
                self.members.append(HipEngine(n_bins, dtype, rank=r, world=R, device=d, tiles=tiles))
            handles = (_lib.c_void_p * R)(*[m._h.value for m in self.members])
            self._create(handles, R)
        except BaseException:
            self.close()
            raise

    def close(self):
        _lib.Handle.close(self)                # the group before its members
        for m in getattr(self, "members", ()):
            m.close()
        self.members = []

    def _each(self, name, *args):
        """Every member's `name`(*args), in rank order."""
        for e in self.members:
            getattr(e, name)(*args)

    def _summed(self, name, *args):
        """The members' `name`(*args) added on the host in rank order: (m0 + m1) + m2 ..."""
        out = getattr(self.members[0], name)(*args)
        for e in self.members[1:]:
            out = out + getattr(e, name)(*args)
        return out

    def layout(self):
        return self.members[0].layout()

    # -- inputs: every member packs its own units from the one input --------------------
    def set_wish_dense(self, matrix, kind, alpha):
        self._each("set_wish_dense", _check_square(matrix, self.n_bins), kind, alpha)

    def set_wish_sparse(self, rows, cols, vals, kind, alpha, KRnorm=None, KRexpected=None):
        self._each("set_wish_sparse", rows, cols, vals, kind, alpha, KRnorm, KRexpected)

    def set_wish_triples(self, dev_triples, kind, alpha, KRnorm=None, KRexpected=None):
        """`dev_triples.per_device`: the triples uploaded once per distinct device."""
        per_device = getattr(dev_triples, "per_device", {dev_triples.device: dev_triples})
        for e in self.members:
            e.set_wish_triples(per_device[e.device], kind, alpha, KRnorm, KRexpected)

    def set_wish_from_coords(self, xstar):
        self._each("set_wish_from_coords", _check_coords(xstar, self.n_bins))

    def set_wish_resident(self, cm, kind, alpha):
        """A resident ContactMap: members on its device pack device to device, members on
        other devices over peer access where the devices allow it; the rest share ONE host
        download of it."""
        dev = cm._resident()
        host = None
        for e in self.members:
            if e.device == dev.device:
                e.set_wish_resident(cm, kind, alpha)
                continue
            # explicit: "without peer access" sends this member through the host, not an error
            rc = e._status("set_wish_from_cm", dev._open(), _KINDS[kind], float(alpha))
            if rc == _lib.BB_OK:
                continue
            if not (rc == _lib.BB_ERR_INVALID and "without peer access" in _lib.last_error()):
                _lib.check(rc, "bb_solver_set_wish_from_cm")
            if host is None:
                host = cm.to_host()
            e.set_wish_dense(host, kind, alpha)

    # -- per-bin steps, weighting: summed on the host in rank order ---------------------
    def degrees(self):
        return self._summed("degrees")

    def set_weight_power(self, q):
        self._each("set_weight_power", q)

    def weight_sums(self):
        return self._summed("weight_sums")

    def set_bin_steps(self, scale):
        self._each("set_bin_steps", scale)

    def score(self, xyz=None):
        """SPEC 2.8 over the whole map: each of the members' two arrays summed in rank order."""
        profile, bins = self.members[0].score(xyz)
        for e in self.members[1:]:
            p, b = e.score(xyz)
            profile, bins = profile + p, bins + b
        return profile, bins

    def loglog(self, xyz=None):
        """SPEC 2.11 over the whole map: the members' sums added in rank order."""
        return self._summed("loglog", xyz)

    def repower(self, p):
        self._each("repower", p)

    def matvec_sq(self, x):
        """(D o D) @ x over the whole map: the members' products summed in rank order (the
        host-driven spectral start)."""
        return self._summed("matvec_sq", x)

    # -- iterations -------------------------------------------------------
    def set_coords(self, x0):
        self._each("set_coords", _check_coords(x0, self.n_bins))

    def set_momentum(self, mu):
        self._each("set_momentum", mu)

    def iterate(self, iters, lr):
        self._call("iterate", int(iters), float(lr))

    def get_coords(self):
        return self.members[0].get_coords()

    def stress_history(self):
        return self.members[0].stress_history()

    def member_coords(self):
        """Every member's coordinates (identical bits: a check, not a result)."""
        return [e.get_coords() for e in self.members]

    def member_stress_histories(self):
        return [e.stress_history() for e in self.members]

    def sync(self):
        self._each("sync")


def _check_square(matrix, n_bins):
    m = numpy.asarray(matrix)
    _square_bins(m.shape)
    if m.shape[0] != n_bins:
        raise ValueError("contact matrix has %d bins, solver was created for %d"
                         % (m.shape[0], n_bins))
    if m.dtype != numpy.float64 or m.strides[1] != 8 or m.strides[0] % 8 or m.strides[0] < 8 * n_bins:
        m = numpy.ascontiguousarray(m, dtype=numpy.float64)
    return m


def _square_bins(shape):
    """The number of bins of a contact matrix of this shape, which has to be n x n."""
    if len(shape) != 2 or shape[0] != shape[1]:
        raise ValueError("contact matrix must be square, got shape %r" % (shape,))
    return int(shape[0])


def _kr_pair(KRnorm, KRexpected, n_bins):
    """The two KR vectors of an input, padded to n_bins and as the pointers the C-ABI takes
    (they keep their arrays alive), or (None, None) without them."""
    if KRnorm is None and KRexpected is None:
        return None, None
    if KRnorm is None or KRexpected is None:
        raise ValueError("KRnorm and KRexpected go together")
    return (_lib.as_f64_ptr(_pad_vector(KRnorm, n_bins)),
            _lib.as_f64_ptr(_pad_vector(KRexpected, n_bins)))


def _pad_vector(v, n):
    """KR vectors have n_bins entries, the matrix n_bins+1 bins: pad with NaN
    (a NaN divisor = no constraint, as for unmappable bins in Rao's files)."""
    v = numpy.asarray(v, dtype=numpy.float64).ravel()
    if v.shape[0] > n:
        raise ValueError("KR vector longer than the number of bins")
    out = numpy.full(n, numpy.nan)
    out[:v.shape[0]] = v
    return out


def _check_coords(x, n_bins):
    x = numpy.ascontiguousarray(x, dtype=numpy.float64)
    if x.shape != (n_bins, 3):
        raise ValueError("coordinates must have shape (%d, 3), got %r" % (n_bins, x.shape))
    if not numpy.all(numpy.isfinite(x)):
        raise ValueError("coordinates must be finite")
    return x


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


def _sum_over_ranks(counts, eng, world):
    """Element-wise sum of an int64 host array over the ranks (world 1: the array); a float
    array is summed in float64 (the weighted degrees of SPEC 2.4.1)."""
    if world <= 1:
        return counts
    import torch
    import torch.distributed as dist
    kind = numpy.float64 if numpy.asarray(counts).dtype.kind == "f" else numpy.int64
    t = torch.from_numpy(numpy.ascontiguousarray(counts, dtype=kind))
    if dist.get_backend() == "nccl":
        t = t.to(torch.device("cuda", eng.device))
        dist.all_reduce(t)
        return t.cpu().numpy()
    dist.all_reduce(t)
    return t.numpy()


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


def allreduce_exchange(t):
    """Sum a device-resident exchange tensor over all ranks, in place: one
    all-reduce of 3*n_pad+2 elements (backend nccl = RCCL, over xGMI)."""
    import torch.distributed as dist
    dist.all_reduce(t, op=dist.ReduceOp.SUM)


def allreduce_exchange_host(eng):
    """The same sum for a host-memory collective (backend gloo: CPU rehearsals,
    tests, 2 ranks sharing one GPU): read the buffer through the C-ABI, reduce
    on the host in float64, write it back.  Transport only -- the kernels on
    either side are the same ones the RCCL path runs."""
    import torch
    import torch.distributed as dist
    host = torch.from_numpy(eng.read_exchange())
    dist.all_reduce(host, op=dist.ReduceOp.SUM)
    eng.write_exchange(host.numpy())


def _dist_state(distributed):
    """(rank, world) of the running torch.distributed job, or (0, 1)."""
    if distributed is False:
        return 0, 1
    if distributed is None:
        # auto: a process that runs a torch.distributed job has imported it already;
        # importing torch here just to find that out costs the first fit() 0.7 s
        dist = sys.modules.get("torch.distributed")
        if dist is None:
            return 0, 1
    else:
        import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    if distributed:
        raise RuntimeError("distributed=True but torch.distributed is not initialised")
    return 0, 1


def _check_devices(devices, n_gpus, device, distributed):
    """The device list of StructureSolver(devices=, n_gpus=), validated without a GPU, or
    None when neither is given."""
    if devices is None and n_gpus is None:
        return None
    if devices is not None and n_gpus is not None:
        raise ValueError("give devices or n_gpus, not both")
    if device is not None:
        raise ValueError("give device or devices / n_gpus, not both")
    if distributed:
        raise ValueError("devices / n_gpus drive several GPUs from one process; distributed=True "
                         "runs one GPU per process")
    if n_gpus is not None:
        if isinstance(n_gpus, bool) or int(n_gpus) != n_gpus or int(n_gpus) < 1:
            raise ValueError("n_gpus must be a positive integer")
        devices = list(range(int(n_gpus)))
    devices = list(devices)
    if not devices:
        raise ValueError("devices must name at least one device")
    for d in devices:
        if isinstance(d, bool) or not isinstance(d, (int, numpy.integer)) or d < 0:
            raise ValueError("devices must be non-negative device indices, got %r" % (d,))
    if len(devices) > 16:
        raise ValueError("devices: at most 16 members")
    return [int(d) for d in devices]


def _check_complete(complete):
    """The `complete=` argument of fit / fit_many / fit_triples, checked before any device call."""
    if complete is not None and complete != "shortest_path":
        raise ValueError("complete must be None or 'shortest_path', got %r" % (complete,))


@contextlib.contextmanager
def _teardown(eng):
    """Close the engine when the fit ends, however it ends."""
    try:
        yield
    except BaseException:
        # this rank leaves a multi-rank job in the middle: its peers may sit in a collective
        # on the library's communicator, which must then not go back into the cache for the
        # next fit() to borrow (close() would return it as free)
        if _exchange_state(eng) == "rccl" and hasattr(eng, "comm_abort"):
            try:
                eng.comm_abort()
            except Exception:                  # noqa: BLE001 -- the first error is the one to report
                pass
        raise
    finally:
        eng.close()


class FitScore(object):
    """How well a structure fits a map, from the device's sums (SPEC 2.8, `StructureSolver.score`).

    sums : (n_bins, 9) float64, row k = the constrained pairs of separation j - i = k: pairs,
        sum d, sum delta, sum d^2, sum delta^2, sum d delta, sum (d - delta)^2,
        sum (d - delta)^2 / delta, sum ((d - delta) / delta)^2
    bin_sums : (n_bins, 3) float64, row i = the pairs that hold bin i: pairs, sum (d - delta)^2,
        sum ((d - delta) / delta)^2

    Derived on the host in float64:
    n_pairs : the constrained pairs
    stress : array of 3, S_q of SPEC 2.3.1 for q = 0, 1, 2 -- comparable between fits made
        with different weight_power
    normalized_stress : stress[0] / sum delta^2
    pearson : Pearson r of (d, delta) over the pairs; NaN with fewer than 2 pairs or no variance
    pairs, mean_distance, mean_wish, rms_relative_error : per separation k (int64; the others
        NaN where pairs == 0); rms_relative_error = sqrt(mean ((d - delta) / delta)^2)
    bin_pairs, bin_stress, bin_relative : per bin: its pairs (int64), its sum (d - delta)^2
        (every pair counts at both of its bins: the bins add up to 2 stress[0]) and the rms
        relative error of its pairs (NaN for a bin without pairs)
    """

    def __init__(self, sums, bin_sums):
        self.sums = numpy.ascontiguousarray(sums, dtype=numpy.float64)
        self.bin_sums = numpy.ascontiguousarray(bin_sums, dtype=numpy.float64)
        if self.sums.ndim != 2 or self.sums.shape[1] != 9 or self.bin_sums.shape != (self.sums.shape[0], 3):
            raise ValueError("FitScore: sums must be (n_bins, 9) and bin_sums (n_bins, 3)")
        tot = self.sums.sum(axis=0)
        n, sd, sw, sdd, sww, sdw = (float(v) for v in tot[:6])
        self.n_pairs = int(round(n))
        self.stress = tot[6:9].copy()
        self.normalized_stress = float(tot[6] / sww) if sww > 0 else float("nan")
        # (a variance the rounding of its own sums could have made counts as none: each of the
        # moments is good to n 2^-53 of itself)
        var_d, var_w, noise = n * sdd - sd * sd, n * sww - sw * sw, 8.0 * n * n * 2.0 ** -53
        self.pearson = (float((n * sdw - sd * sw) / numpy.sqrt(var_d * var_w))
                        if self.n_pairs >= 2 and var_d > noise * sdd and var_w > noise * sww
                        else float("nan"))

        def per(total, count):
            return numpy.where(count > 0, total / numpy.where(count > 0, count, 1.0), numpy.nan)
        cnt = self.sums[:, 0]
        self.pairs = numpy.rint(cnt).astype(numpy.int64)
        self.mean_distance = per(self.sums[:, 1], cnt)
        self.mean_wish = per(self.sums[:, 2], cnt)
        self.rms_relative_error = numpy.sqrt(per(self.sums[:, 8], cnt))
        self.bin_pairs = numpy.rint(self.bin_sums[:, 0]).astype(numpy.int64)
        self.bin_stress = self.bin_sums[:, 1].copy()
        self.bin_relative = numpy.sqrt(per(self.bin_sums[:, 2], self.bin_sums[:, 0]))

    def __repr__(self):
        return ("FitScore(n_pairs=%d, stress=%s, normalized_stress=%.6g, pearson=%.6g)"
                % (self.n_pairs, numpy.array2string(self.stress, precision=6),
                   self.normalized_stress, self.pearson))


class StructureSolver(object):
    """Infer 3D bin coordinates from a Hi-C contact matrix (metric MDS).

    Minimises  S(X) = sum_{i<j, c_ij>0} (|x_i - x_j| - delta_ij)^2  with
    delta_ij = c_ij^(-1/alpha), by `n_iter` gradient steps  X <- X - lr * grad S
    (docs/SPEC.md).  With lr = 1/(2 N) and a complete matrix each step equals a
    SMACOF / Guttman-transform step, so the stress never increases.

    Parameters
    ----------
    n_iter : int
        Number of iterations (fixed; there is no convergence test on the device).
    lr : float or 'auto'
        Step size; 'auto' = 1 / (2 * n_bins).
    dtype : 'float32' or 'float64'
        Arithmetic type on the GPU.
    alpha : float, 'auto', ('auto', alpha0), ('auto', alpha0, max_rounds) or
            ('auto', alpha0, max_rounds, tol)
        Count-to-distance exponent, delta = c^(-1/alpha).  'auto' infers it in the fit (SPEC
        2.11): after `n_iter` iterations at alpha0 (3.0) the log-log slope p of fitted on wish
        distance is taken on the device; while |p - 1| > tol (1e-3) and fewer than max_rounds
        (8) rounds have run, the next exponent comes from a secant step on (ln alpha, ln p),
        the resident wish distances are re-exponentiated in place, the structure is rescaled
        and `n_iter` iterations run again.  Then the map is packed once more at `alpha_` and
        `n_iter` iterations run from `alpha_init_`: `structure_` and `stress_` are bit for bit
        those of StructureSolver(alpha=alpha_, ...).fit(X, init=alpha_init_).  The options ride
        in `alpha` (stored normalised; `alpha_start`, `alpha_rounds`, `alpha_tol` read them
        back) so that clones carry them.  For every input of `fit` and `fit_triples`
        (`balance=`, `devices=`, a distributed world: every rank takes the same alpha); `score`
        then uses `alpha_` (ValueError before a fit).  ValueError with kind='wish' (no counts),
        complete='shortest_path' and init='landmark' (distances that are sums along paths
        cannot be re-exponentiated) and for `fit_many`; ValueError for a map with fewer than 3
        usable pairs or whose counts do not vary; RuntimeError when a slope is <= 0 or a round's
        coordinates are not finite (the fit diverged).  Exact on
        noise-free maps; on Poisson-sampled counts whose zero cells are dropped the estimate is
        biased upwards (3.27 for a true 3; 3.58 with weight_power=2): the zeros are truncated
        and the estimator has no model for them.
    kind : 'counts' or 'wish'
        Whether the input matrix holds contact counts or wish distances.
    seed : int
        Seed of the default initial coordinates (numpy default_rng standard normal).
    tol : float or None
        None: exactly n_iter steps.  Otherwise stop as soon as the relative stress
        decrease of one step is <= tol, checked every `check_every` steps (n_iter is
        then the maximum); `n_iter_` tells how many were run.
    init : 'random', 'spectral', 'landmark', ('landmark', n_landmarks) or
           ('landmark', n_landmarks, landmark_weight)
        Start used when `fit()` gets no `init=` array: seeded standard normal, or
        classical MDS computed on the device (`spectral_init`), or -- for the sparse inputs,
        `fit_triples` and `fit(scipy.sparse)` -- landmark MDS over shortest paths on the stored
        pairs (`landmark_start`, SPEC 2.5.4), which gives a map with counts only between nearby
        bins its global fold without the dense matrix.  'landmark' takes 64 landmarks; the
        tuple form another number, an int in [4, 1024] (`n_landmarks` reads it back; it is part
        of `init` and not a constructor argument of its own, so that clones carry it).  The
        start is computed once, on devices[0] of `devices=` or on the rank's own device, under
        this solver's kind and alpha and the bias the fit uses (KR vectors, `balance=`), and
        handed to the unchanged fit as `init=`; `landmarks_` and `landmark_placed_` tell which
        bins were landmarks and which were placed.  Not for dense inputs or a ContactMap
        (`complete='shortest_path'` is their route, or init='spectral'), not with
        `complete='shortest_path'`, `fit_many`, or an engine without a device: ValueError.
        The stored pairs alone do not hold the fold for ever (SPEC 2.5.4): few iterations, or
        ('landmark', n_landmarks, landmark_weight) with landmark_weight > 0 (SPEC 2.5.5): the
        kept landmarks' geodesic rows stay in the fit as constraints, every term weighted
        landmark_weight * D^-weight_power, and hold the fold over any number of iterations
        (`landmark_weight` reads it back; 0, the default, is the fit without them bit for bit).
        It needs degree_steps=True (a landmark touches about N terms: ValueError otherwise) and
        ONE device (`devices=` / `n_gpus` of several, a distributed world > 1: ValueError);
        `stress_` is then the total of stored pairs and landmark terms, `anchor_stress_` the
        latter's share at the end, `landmark_terms_` their number.  An `init=` array given to
        the call replaces the start only; the constraints stay.  The anchored fit reduces the
        stress of the stored pairs less than the free one.
    degree_steps : bool
        A step per bin from the map itself (SPEC 2.4.1): bin i steps by 1 / (2 (deg_i + 1)),
        deg_i = the number of pairs that constrain it (counted on the device, summed over
        the ranks), instead of one step for all (`lr='auto'`: 1 / (2 N), the step of a
        COMPLETE map).  For incomplete maps -- blocked-sparse input, a whole genome whose
        chromosomes differ in size, real maps whose long-range pairs have no contact -- that
        is each bin's own Guttman-like step: a genome-like map converges in about a third
        of the iterations.  A float `lr` is then the step of the bin with the most partners.
        A complete map: no effect.  With weight_power > 0 the weighted degree
        s_i = sum_j delta_ij^-q takes the place of deg_i: bin i steps by 1 / (2 s_i).
    weight_power : 0, 1 or 2
        Weight w = delta^-q of each pair's squared residual (SPEC 2.3.1).  0: raw stress, where
        the long-range pairs (largest, noisiest delta) dominate.  1: Sammon stress, a middle
        ground.  2: relative stress, sum ((d - delta) / delta)^2, every pair's relative error
        counts alike -- the local structure, the best-measured part of a Hi-C map, gets its
        share.  With q > 0, lr='auto' is 1 / (2 max_i s_i), s_i the weighted degree; `stress_`
        reports the weighted stress.  float32 refuses (ValueError) a map whose largest s_i
        exceeds 2^60.
    spectral_iter, spectral_tol : int, float
        The spectral start's block power iteration makes at most `spectral_iter` products
        and ends once B V lies within `spectral_tol` (relative) of span(V); 0 = always
        `spectral_iter` products.  `spectral_iterations_` tells how many were made.
    momentum : float in [0, 1)
        Heavy-ball coefficient mu: V <- mu V - lr g, X <- X + V.  0 = plain steps.
    device : int or None
        HIP device index; None = LOCAL_RANK (distributed) or 0.
    devices : list of int or None
        Several GPUs driven from THIS process, no torch.distributed job needed: member r of
        the group plays rank r of world len(devices) on devices[r], packs only its own units
        from the one input, and a host thread per member enqueues its iterations; the
        partials are summed in rank order by an exchange ordered with HIP events
        (`GroupEngine`, `bb_group_*`), bit-identical to the process-per-rank peer exchange
        (two-launch form) at the same world size.  One entry: as `device=`.  A device may
        repeat -- members then take turns on it: a rehearsal, the one form a one-GPU box can
        run.  Not with `device`, `n_gpus`, `distributed=True` or inside a torch.distributed
        job; not for `fit_many`.
    n_gpus : int or None
        Shorthand for devices=list(range(n_gpus)).
    distributed : bool or None
        None: shard over the ranks of an initialised torch.distributed job if
        there is one.  Every rank passes the same matrix and gets the same result.

    Attributes
    ----------
    structure_ : numpy.ndarray, shape (n_bins, 3), float64
    stress_ : numpy.ndarray, shape (n_iter,) -- stress BEFORE each step
    n_bins_, lr_ : the problem size and the step actually used
    exchange_ : how the ranks summed their partial gradients ('rccl', 'peer', 'torch',
        'host', 'group' for devices=), None on one rank.  Results are reproducible bit for
        bit for a given transport; fit() never picks one by timing (that is bench.py's trial).
    devices_ : the devices of a `devices=` / `n_gpus=` fit, member by member; else None.
    alpha_ : the exponent of the fit: the inferred one under alpha='auto', else `alpha`.
    alpha_rounds_ : (rounds, 5) float64, per round of the search alpha_r, the slope p_r, the
        intercept a_r, the log-log correlation, the iterations run; (0, 5) for a float alpha.
    alpha_converged_ : whether the search ended by |p - 1| <= tol (True for a float alpha).
    alpha_init_ : (n_bins, 3), the start of the last fit under 'auto'; None for a float alpha.

    Failure on several ranks.  A rank that fails mid-fit raises, and takes the library's
    communicator out of the cache (its peers may still sit in a collective on it).  With
    the peer exchange ('peer', BB_COMM=peer or a trial) in its one-launch form every wave
    decides for its own 64 coordinates, so a rank that dies IN THE MIDDLE of an exchange can
    leave its peers with part of a step applied: their fit() then raises too
    (`peer_status`), and the coordinates of a solver that raised are not a result.  Nothing
    of a rank that is late or gone ever arrives, so nothing is applied; the two-launch form
    (ranks sharing a GPU, BB_PEER_FUSED=0) applies a step whole or not at all.
    """

    def __init__(self, n_iter=100, lr="auto", dtype="float32", alpha=3.0, kind="counts",
                 seed=0, device=None, distributed=None, engine=None, momentum=0.0,
                 init="random", tol=None, check_every=10, spectral_iter=40, spectral_tol=1e-3,
                 degree_steps=False, weight_power=0, devices=None, n_gpus=None):
        if dtype not in _DTYPES:
            raise ValueError("dtype must be 'float32' or 'float64'")
        if kind not in _KINDS:
            raise ValueError("kind must be 'counts' or 'wish'")
        if int(n_iter) < 0:
            raise ValueError("n_iter must be >= 0")
        if int(n_iter) > (1 << 20):
            raise ValueError("n_iter is limited to 2**20: the per-iteration stress history "
                             "lives on the device (include/blueberry_hip.h, bb_solver_iterate)")
        if not (lr == "auto" or float(lr) > 0):
            raise ValueError("lr must be positive or 'auto'")
        alpha = _check_alpha(alpha)
        if isinstance(alpha, tuple):
            if kind == "wish":
                raise self._auto_refusal("infers the exponent of counts: kind='wish' holds wish "
                                         "distances, which have none")
            if init == "landmark" or (isinstance(init, tuple) and init[:1] == ("landmark",)):
                raise self._auto_refusal("does not go with init='landmark': the landmark start and "
                                         "its geodesic rows are made of the wish distances of one "
                                         "alpha, which the search changes")
        if not 0.0 <= float(momentum) < 1.0:
            raise ValueError("momentum must be in [0, 1)")
        self.momentum = float(momentum)
        if tol is not None and not float(tol) > 0:
            raise ValueError("tol must be positive or None")
        if int(check_every) < 1:
            raise ValueError("check_every must be >= 1")
        self.tol, self.check_every = (None if tol is None else float(tol)), int(check_every)
        if isinstance(init, tuple) and len(init) in (2, 3) and init[0] == "landmark":
            init = ("landmark", _check_n_landmarks(init[1])) + tuple(
                _check_landmark_weight(w) for w in init[2:])
        elif not (isinstance(init, str) and init in ("random", "spectral", "landmark")):
            raise ValueError("init must be 'random', 'spectral', 'landmark', ('landmark', "
                             "n_landmarks) or ('landmark', n_landmarks, landmark_weight) (or pass "
                             "init= to fit())")
        self.init = init
        if int(spectral_iter) < 0 or not 0.0 <= float(spectral_tol) < 1.0:
            raise ValueError("need spectral_iter >= 0 and 0 <= spectral_tol < 1")
        self.spectral_iter, self.spectral_tol = int(spectral_iter), float(spectral_tol)
        self.degree_steps = bool(degree_steps)
        if isinstance(weight_power, bool) or weight_power not in (0, 1, 2):
            raise ValueError("weight_power must be 0, 1 or 2")
        self.weight_power = int(weight_power)
        self.n_iter, self.lr, self.dtype, self.alpha, self.kind, self.seed = (
            int(n_iter), lr, dtype, alpha, kind, int(seed))
        self.device, self.distributed = device, distributed
        # Engine factory: the HIP engine unless a test injects another one to
        # rehearse the multi-rank orchestration without a GPU.
        self._engine_factory = engine if engine is not None else HipEngine
        self.devices, self.n_gpus = devices, n_gpus
        self._group = _check_devices(devices, n_gpus, device, distributed)
        if self._group is not None and len(self._group) == 1:
            self.device = self._group[0]           # one entry: as device=
        elif self._group is not None and engine is not None:
            raise ValueError("devices= runs HIP engines of its own; it takes no engine=")
        self._anchor = None                 # (rows, kept) between the landmark start and the fit
        if self.landmark_weight > 0.0:
            if not self.degree_steps:
                raise ValueError("landmark_weight > 0 needs degree_steps=True: a landmark touches "
                                 "about landmark_weight * N terms, so the one global step its "
                                 "weighted degree allows, 1 / (2 landmark_weight N), would slow "
                                 "every bin down to it (docs/SPEC.md 2.5.5)")
            self._check_anchor_devices(None)

    def _pick_device(self, world):
        if self.device is not None:
            return int(self.device)
        return int(os.environ.get("LOCAL_RANK", "0")) if world > 1 else 0

    @staticmethod
    def _auto_refusal(why):
        return ValueError("alpha='auto' %s; give a float alpha" % why)

    @property
    def alpha_auto(self):
        """Whether the exponent is inferred in the fit (alpha='auto' in any form, SPEC 2.11)."""
        return isinstance(self.alpha, tuple)

    @property
    def alpha_start(self):
        """alpha0 of alpha=('auto', alpha0, ...) (3.0 for 'auto'); a float alpha: that alpha."""
        return self.alpha[1] if self.alpha_auto else self.alpha

    @property
    def alpha_rounds(self):
        """max_rounds of alpha=('auto', alpha0, max_rounds, ...) (8); None for a float alpha."""
        return self.alpha[2] if self.alpha_auto else None

    @property
    def alpha_tol(self):
        """tol of alpha=('auto', alpha0, max_rounds, tol) (1e-3); None for a float alpha."""
        return self.alpha[3] if self.alpha_auto else None

    def _pack_alpha(self):
        """The exponent a map is packed under outside a search: the float alpha, or alpha_ of
        the last 'auto' fit (ValueError before one)."""
        if not self.alpha_auto:
            return self.alpha
        if getattr(self, "alpha_", None) is None:
            raise ValueError("alpha='auto': no exponent inferred yet (alpha_ is set by a fit)")
        return self.alpha_

    @property
    def n_landmarks(self):
        """The landmarks of init='landmark' (64) / ('landmark', n); None for another init."""
        if self.init == "landmark":
            return 64
        return self.init[1] if isinstance(self.init, tuple) else None

    @property
    def landmark_weight(self):
        """The weight of the landmark constraints (SPEC 2.5.5): the third entry of
        init=('landmark', n_landmarks, landmark_weight); 0.0 (none) for every other init."""
        return self.init[2] if isinstance(self.init, tuple) and len(self.init) == 3 else 0.0

    def _landmark_refusal(self, why, instead):
        return ValueError("init='landmark' %s; use %s" % (why, instead))

    def _check_anchor_devices(self, world):
        """Landmark constraints (landmark_weight > 0) run on one device: a group of several, or
        -- `world` given -- a torch.distributed job of several ranks, is refused."""
        if self.landmark_weight > 0.0 and ((self._group is not None and len(self._group) > 1)
                                           or (world is not None and world > 1)):
            raise self._landmark_refusal("with landmark_weight > 0 keeps its constraints on one "
                                         "device (several devices are not covered)",
                                         "one device, or landmark_weight = 0")

    def _check_landmark_route(self, complete):
        """The refusals of a landmark start that need no device (the caller has a sparse input)."""
        if complete is not None:
            raise self._landmark_refusal("does not go with complete='shortest_path', which "
                                         "determines the fold itself", "init='random' or 'spectral'")
        if not hasattr(self._engine_factory, "set_wish_triples"):
            raise self._landmark_refusal("runs on the device and this solver's engine has none",
                                         "init='spectral'")
        if self.landmark_weight > 0.0:
            self._check_anchor_devices(1 if self._group is not None else _dist_state(self.distributed)[1])

    def _landmark_wanted(self, init):
        """Whether a call with this `init=` goes the landmark route: for the start (no init
        given), and -- an array replaces only the start -- for the constraints."""
        return self.n_landmarks is not None and (init is None or self.landmark_weight > 0.0)

    def _landmark_init(self, dev, n_bins, KRnorm, KRexpected):
        """The landmark start of the map in `dev` (a DeviceTriples) under this solver's kind and
        alpha and the fit's KR vectors; `landmarks_` and `landmark_placed_` stay on the solver.
        With landmark_weight > 0 the geodesic rows stay open for the fit (`_anchor`), which hands
        them to its engine and closes them."""
        keep = self.landmark_weight > 0.0
        self._drop_anchor()
        start, info = landmark_start(dev, dev.resolution, n_bins, n_landmarks=self.n_landmarks,
                                     kind=self.kind, alpha=self.alpha, KRnorm=KRnorm,
                                     KRexpected=KRexpected, seed=self.seed, return_info=True,
                                     keep_rows=keep)
        self.landmarks_, self.landmark_placed_ = info.landmarks_, info.placed_
        if keep:
            self._anchor = (info.rows_, info.kept_)
        return start

    def _drop_anchor(self):
        if self._anchor is not None:
            self._anchor[0].close()
            self._anchor = None

    def _take_anchor(self, eng, world):
        """The rows `_landmark_init` kept, copied into the engine (which then owns its copy)
        and closed."""
        if self._anchor is None:
            return
        try:
            self._check_anchor_devices(world)
            if not hasattr(eng, "set_anchors"):
                raise self._landmark_refusal("with landmark_weight > 0 needs an engine that holds "
                                             "the constraints on the device", "HipEngine")
            eng.set_anchors(self._anchor[0], self._anchor[1], self.landmark_weight)
        finally:
            self._drop_anchor()

    def fit(self, X, init=None, complete=None):
        """Solve for the structure of `X`: a ContactMap, a square ndarray, or a
        scipy.sparse matrix (symmetric; either triangle is enough; of several
        COO entries for one pair the last is kept) -- the sparse form never builds
        the dense matrix.

        complete : None or 'shortest_path'
            None: pairs without a contact are no constraint (SPEC 2.1).  'shortest_path': the
            map is first completed on the device by graph shortest paths over its wish
            distances (SPEC 2.1.1, `ContactMap.shortest_paths` with this solver's `kind` and
            `alpha`) -- what a real Hi-C map, with counts only between nearby bins, needs for
            its global fold to be determined -- and the fit is that of
            `StructureSolver(kind='wish', ...).fit(completed)`, dense tiles, bit for bit.
            `completed_unreachable_pairs_` tells how many pairs stayed without a path.  With
            `devices=[...]` the completion runs once on devices[0]; inside a torch.distributed
            job every rank completes the same input on its own GPU.  The dense matrix and a
            work matrix of its size must fit on one device: a whole-genome blocked-sparse map
            (720 GB dense at 10 kb) cannot be completed this way (MemoryError); init='landmark'
            (SPEC 2.5.4) is the route of such a map to its global fold."""
        _check_complete(complete)
        self._check_auto_route(complete)
        if self._landmark_wanted(init):
            try:
                start = self._landmark_init_of_map(X, complete)
                source, n = self._map_source(X)
                return self._fit_impl(source, n, start if init is None else init, None, None)
            finally:
                self._drop_anchor()
        if complete is None:
            source, n = self._map_source(X)
            return self._fit_impl(source, n, init, None, None)
        cm = self._completed(X)
        self.completed_unreachable_pairs_ = cm.unreachable_pairs_
        source, n = self._map_source(cm)
        return self._fit_impl(source, n, init, None, None, kind="wish")

    def _check_auto_route(self, complete):
        if self.alpha_auto and complete is not None:
            raise self._auto_refusal("does not go with complete='shortest_path': the completed "
                                     "distances are sums along paths, not a power of a count, so "
                                     "they cannot be re-exponentiated")

    def _landmark_init_of_map(self, X, complete):
        """fit(X) under init='landmark': the start of a scipy.sparse X, whose COO entries are the
        triples [row, col, value] at resolution 1 over N - 1 bins (an entry that is not finite is
        no constraint there and no edge here); any other input is refused."""
        matrix = X if hasattr(X, "tocoo") else None     # (a ContactMap's matrix is never read)
        if matrix is None:
            raise self._landmark_refusal("needs a sparse input (fit_triples, or fit of a "
                                         "scipy.sparse matrix), not a dense array or a ContactMap",
                                         "complete='shortest_path' or init='spectral'")
        self._check_landmark_route(complete)
        coo = matrix.tocoo()
        n = _square_bins(coo.shape)
        vals = numpy.asarray(coo.data, dtype=numpy.float64)
        triples = numpy.stack([coo.row.astype(numpy.float64), coo.col.astype(numpy.float64),
                               numpy.where(numpy.isfinite(vals), vals, 0.0)], axis=1)
        with _resident_triples(triples, 1, [self._completion_device()]) as dev:
            return self._landmark_init(dev, n - 1, None, None)

    def _completion_device(self):
        """Where a fit's completion runs: devices[0] of a group, else this rank's device."""
        devices = self._group_devices()
        if devices:
            return devices[0]
        return self._pick_device(_dist_state(self.distributed)[1])

    def _completed(self, X, device=None):
        """The shortest-path completion of one input map under this solver's kind and alpha,
        as a resident ContactMap of wish distances."""
        from .datatypes import complete_map
        return complete_map(X, kind=self.kind, alpha=self.alpha,
                            device=self._completion_device() if device is None else device)

    # -- the stages fit() and fit_many() share -----------------------------------------
    def _map_source(self, X, sparse=True):
        """(source, n_bins) of one input map.  source is X itself for a ContactMap whose
        matrix lives in HBM (packed device to device; only its shape is read), a COO matrix
        for scipy.sparse input (`sparse` false -- fit_many, which packs dense blocks -- takes
        it as an array), else the host matrix as an ndarray."""
        if getattr(X, "is_resident", False) and hasattr(self._engine_factory, "set_wish_from_cm"):
            return X, _square_bins(X.shape)
        matrix = getattr(X, "matrix", X)
        if sparse and hasattr(matrix, "tocoo"):    # any scipy.sparse matrix
            matrix = matrix.tocoo()
        else:
            matrix = numpy.asarray(matrix)
        return matrix, _square_bins(matrix.shape)

    def _default_start(self, n):
        return numpy.random.default_rng(self.seed).standard_normal((n, 3))

    def _one_step(self, n):
        """The one step for all bins of a map of n bins: lr='auto' is SPEC 2.4's 1 / (2 n)."""
        return 1.0 / (2.0 * n) if self.lr == "auto" else float(self.lr)

    def _fitted(self, structure, who):
        """`structure`, or `structure_` of the last fit where none is given (ValueError before one)."""
        if structure is None:
            structure = getattr(self, "structure_", None)
            if structure is None:
                raise ValueError("%s: no structure given and none fitted yet (structure_)" % who)
        return structure

    def _bin_sums(self, eng, world):
        """What the per-bin steps of SPEC 2.4.1 are made from, summed over the ranks: the
        weighted degrees (weight_power, which is switched on here), the degrees
        (degree_steps), or None for the one step of SPEC 2.4."""
        if self.weight_power:
            eng.set_weight_power(self.weight_power)
            sums = _sum_over_ranks(eng.weight_sums(), eng, world)
        elif self.degree_steps:
            sums = _sum_over_ranks(eng.degrees(), eng, world)
        else:
            return None
        if getattr(eng, "anchored", False):
            # SPEC 2.5.5: the landmark terms join the (weighted) degrees, as float64
            sums = numpy.asarray(sums, dtype=numpy.float64) + eng.anchor_sums()
        return sums

    def _steps(self, sums, n, anchored=False):
        """(lr, scale) for one map of n bins from its slice of `_bin_sums`: `weighted_steps`
        (weighted stress, or `anchored`: the sums hold landmark terms, SPEC 2.5.5) or
        `degree_step_factors`, a float `lr` being the step of the best-connected bin."""
        if self.weight_power or anchored:
            return weighted_steps(sums, n, self.dtype, self.lr, self.degree_steps)
        lr, scale = degree_step_factors(sums)
        return (lr if self.lr == "auto" else float(self.lr)), scale

    def _iterate(self, step, history, converged):
        """`n_iter` iterations through step(k).  With `tol` (early stop) they go in chunks
        of `check_every`: after each the stress history is read back (one sync) and the
        loop ends once converged(history()).  Every rank sees the same all-reduced stress,
        so all ranks stop at the same iteration."""
        if self.tol is None:
            step(self.n_iter)
            return
        done = 0
        while done < self.n_iter:
            k = min(self.check_every, self.n_iter - done)
            step(k)
            done += k
            if converged(history()):
                break

    def _params(self):
        """Every argument of the constructor as this solver holds it now."""
        import inspect
        p = {k: getattr(self, k) for k in inspect.signature(type(self).__init__).parameters
             if k not in ("self", "engine")}
        p["engine"] = None if self._engine_factory is HipEngine else self._engine_factory
        if self._group is not None:
            p["device"] = None                     # (set from a one-entry devices=)
        return p

    def _clone(self, **overrides):
        """A solver with this one's parameters, but for `overrides`."""
        return type(self)(**dict(self._params(), **overrides))

    def _fit_impl(self, matrix, n, init, KRnorm, KRexpected, kind=None):
        kind = self.kind if kind is None else kind      # 'wish' for a completed map
        eng, world, devices, pack = self._engine_for(matrix, n)
        lr = self._one_step(n)
        if init is None and self.init == "random":
            init = self._default_start(n)
        auto = self.alpha_auto
        if auto and not (hasattr(eng, "loglog") and hasattr(eng, "repower")):
            eng.close()
            raise self._auto_refusal("needs an engine with the log-log pass and the "
                                     "re-exponentiation (HipEngine)")
        with _teardown(eng):
            pack(kind, KRnorm, KRexpected, self.alpha_start)
            self._take_anchor(eng, world)
            anchored = bool(getattr(eng, "anchored", False))
            sums = self._bin_sums(eng, world)
            if sums is not None:
                lr, scale = self._steps(sums, n, anchored)
                if scale is not None:
                    eng.set_bin_steps(scale)
            on_device = False
            if init is None:
                # 'spectral'.  The whole block power iteration stays on the device -- on one
                # rank, and on several once they have their exchange (peer arenas or the
                # library's communicator: the per-rank products are then summed where they
                # are).  Its Cholesky-QR needs an iterate of full column rank; maps it cannot
                # take -- fewer than 4 bins (centring leaves at most 2 directions), an empty
                # or unconstrained map -- and transports that sum on the host (gloo, torch)
                # go through the host-driven form below, so the same input runs everywhere.
                v0 = self._default_start(n)
                if world > 1:
                    eng.set_coords(v0)             # (a trial in select_exchange wants a start)
                    select_exchange(eng, lr)
                device_form = hasattr(eng, "spectral_init_device") and n >= 4 and (
                    world == 1 or _exchange_state(eng) in ("peer", "rccl"))
                if device_form:
                    try:
                        info = eng.spectral_init_device(self.spectral_iter, v0, tol=self.spectral_tol)
                        self.spectral_iterations_ = info[0] if info else self.spectral_iter
                        on_device = True
                    except RankDeficient:
                        pass
                    if world > 1:
                        if _exchange_state(eng) == "peer":
                            eng.peer_status()
                        on_device = _all_ranks(on_device)
            if not on_device:
                if init is None:                   # 'spectral', host-driven
                    init, self.spectral_iterations_ = spectral_init(
                        eng, n, world, n_iter=self.spectral_iter, seed=self.seed,
                        tol=self.spectral_tol, return_iterations=True)
                eng.set_coords(init)
            if self.momentum:
                eng.set_momentum(self.momentum)
            if world > 1:
                select_exchange(eng, lr)
            # converged: the relative decrease of the last step is <= tol (never at stress 0)
            def run(lr):
                self._iterate(lambda k: run_iterations(eng, k, lr, world), eng.stress_history,
                              lambda h: h.size >= 2 and h[-2] > 0
                              and abs(h[-2] - h[-1]) <= self.tol * h[-2])
            run(lr)
            if auto:
                lr = self._alpha_search(eng, world, n, run, lambda a: pack(kind, KRnorm, KRexpected, a))
            else:
                self.alpha_, self.alpha_rounds_ = self.alpha, numpy.zeros((0, 5))
                self.alpha_converged_, self.alpha_init_ = True, None
            if _exchange_state(eng) == "peer":
                eng.peer_status()              # raises if a peer wait ran into its time limit
            self.exchange_ = _exchange_state(eng)
            self.structure_ = eng.get_coords()
            self.stress_ = eng.stress_history()
            if self.n_landmarks is not None:
                self.anchor_stress_ = eng.anchor_stress() if anchored else 0.0
                self.landmark_terms_ = eng.anchor_info()[1] if anchored else 0
        self.devices_ = devices
        self.n_bins_, self.lr_, self.n_iter_ = n, lr, int(self.stress_.shape[0])
        return self

    def _engine_for(self, matrix, n):
        """The engine one input map runs on, the map not yet in it: (eng, world, devices, pack).
        pack(kind, KRnorm, KRexpected) packs the map as the form of `matrix` asks -- resident
        ContactMap, device triples, scipy.sparse (blocked-sparse: only the tiles that hold an
        entry exist on the device) or a host matrix.  The caller closes the engine."""
        resident = getattr(matrix, "is_resident", False)
        triples = getattr(matrix, "is_triples", False)
        sparse = hasattr(matrix, "row") and not resident
        if n < 2:
            raise ValueError("need at least 2 bins (the contact map is empty)" if n == 0 else
                             "need at least 2 bins")
        devices = self._group_devices()                 # checked for one entry as well
        group = devices if devices and len(devices) > 1 else None
        rank, world = (0, 1) if devices else _dist_state(self.distributed)
        tiles = None
        if sparse:
            keep = matrix.row != matrix.col
            rows, cols, vals = matrix.row[keep], matrix.col[keep], matrix.data[keep]
            tiles = tiles_from_entries(n, rows, cols, self.dtype)
        elif triples:
            tiles = matrix.tiles(n, self.dtype)
        if group:
            eng = GroupEngine(n, self.dtype, group, tiles=tiles)
        else:
            eng = self._engine_factory(n, self.dtype, rank=rank, world=world,
                                       device=self._pick_device(world), tiles=tiles)

        def pack(kind, KRnorm, KRexpected, alpha=None):
            alpha = self._pack_alpha() if alpha is None else alpha
            if resident:
                eng.set_wish_resident(matrix, kind, alpha)
            elif triples:
                eng.set_wish_triples(matrix, kind, alpha, KRnorm, KRexpected)
            elif sparse:
                eng.set_wish_sparse(rows, cols, vals, kind, alpha, KRnorm, KRexpected)
            else:
                eng.set_wish_dense(matrix, kind, alpha)
        return eng, world, devices, pack

    def _alpha_search(self, eng, world, n, run, pack_at):
        """SPEC 2.11 on the engine of a fit whose round 0 (packed at alpha_start, `n_iter`
        iterations from the fit's start) has just run: the rounds of the search -- log-log sums,
        slope, next exponent, the units re-exponentiated on the device, the structure rescaled
        -- and then the fit proper at alpha_: the map packed once more from the input by
        pack_at(alpha), the steps recomputed, `n_iter` iterations from alpha_init_.  run(lr)
        iterates; returns the lr of that last fit.  Every rank takes the same decisions: the
        sums are the same on all of them."""
        def steps():
            lr = self._one_step(n)
            sums = self._bin_sums(eng, world)
            if sums is not None:
                lr, scale = self._steps(sums, n)
                eng.set_bin_steps(scale)            # (None: one step for all again)
            return lr
        _, alpha, max_rounds, tol = self.alpha
        rounds, converged = [], False
        while True:
            x = eng.get_coords()
            if not numpy.isfinite(x).all():
                # (a distance that is not a number has no logarithm either: the sums would count
                # it with the pairs at d = 0 and the slope would speak of too few pairs)
                raise RuntimeError("alpha='auto': the fit diverged in round %d at alpha = %.6g (its "
                                   "coordinates are not finite): a smaller lr, or a fixed alpha"
                                   % (len(rounds), alpha))
            iters = int(eng.stress_history().shape[0])
            totals =_sum_over_ranks(loglog_totals(eng.loglog()), eng, world)
            p, a, r_log, ubar, vbar = loglog_slope(totals)
            rounds.append((alpha, p, a, r_log, float(iters)))
            converged = abs(p - 1.0) <= tol
            if converged or len(rounds) == max_rounds:
                break
            nxt = next_alpha(rounds)
            power = alpha / nxt
            eng.repower(power)
            lr = steps()
            eng.set_coords(math.exp(power * ubar - vbar) * x)
            alpha = nxt
            run(lr)
        self.alpha_, self.alpha_converged_ = float(alpha), bool(converged)
        self.alpha_rounds_ = numpy.array(rounds, dtype=numpy.float64)
        self.alpha_init_ = math.exp(ubar - vbar) * x
        pack_at(self.alpha_)
        lr = steps()
        eng.set_coords(self.alpha_init_)
        run(lr)
        return lr

    def score(self, X, structure=None):
        """How well a structure fits the map `X` (SPEC 2.8): a `FitScore`.  `X` takes every
        form `fit` takes and is packed the same way, under this solver's kind, alpha, dtype and
        devices; no iteration runs -- one pass over the packed map forms float64 sums per
        genomic separation and per bin, summed over the ranks of a torch.distributed job or
        the members of `devices=`.  structure: (n_bins, 3); None: `structure_` of the last fit.
        The score is against the pairs `X` holds: to score against a completed map, pass
        `ContactMap.shortest_paths(...)` to a kind='wish' solver.  Comparable across
        weight_power: `FitScore.stress` holds all three S_q."""
        source, n = self._map_source(X)
        xyz = _check_coords(self._fitted(structure, "score"), n)
        eng, world, _, pack = self._engine_for(source, n)
        with _teardown(eng):
            pack(self.kind, None, None)
            profile, bins = eng.score(xyz)
            profile = _sum_over_ranks(profile, eng, world)
            bins = _sum_over_ranks(bins, eng, world)
        return FitScore(profile, bins)

    def compare(self, B, A=None, **kw):
        """This fit against another structure `B` of the same bins (SPEC 2.10): a
        `StructureComparison`, `compare_structures(A, B, **kw)` with A = `structure_` of the last
        fit unless given -- B is laid onto A."""
        from .compare import compare_structures
        return compare_structures(self._fitted(A, "compare"), B, **kw)

    def _group_devices(self):
        """The devices of a devices= / n_gpus= fit (one entry included), checked against this
        process (device count, no torch.distributed job), or None without them."""
        if self._group is None:
            return None
        dist = sys.modules.get("torch.distributed")      # never imported here
        if dist is not None and dist.is_available() and dist.is_initialized():
            raise ValueError("devices= drives several GPUs from one process; inside a "
                             "torch.distributed job every rank runs its own GPU (leave devices "
                             "unset)")
        count = _lib.c_int()
        _lib.check(_lib.load().bb_device_count(count), "bb_device_count")
        bad = [d for d in self._group if d >= count.value]
        if bad:
            raise ValueError("devices: index %d is out of range (%d HIP devices)"
                             % (bad[0], count.value))
        return list(self._group)

    def _balance_on(self, source, n_bins, args, want_expected):
        """fit_triples(balance=...): the bias (and the expected, or all ones) of `source`, a
        DeviceTriples or a ContactMap; the results kept on the solver."""
        if getattr(source, "is_triples", False):
            bias = source.balance(n_bins, **args)
            e = source.expected(n_bins, bias) if want_expected else None
        else:
            bias = source.balance(**args)
            e = source.expected() if want_expected else None
        self.bias_, self.balance_masked_ = bias, source.balance_masked_
        self.balance_iterations_ = source.balance_iterations_
        self.balance_converged_ = source.balance_converged_
        self.balance_variance_ = source.balance_variance_
        if want_expected:
            self.expected_ = e
        return bias, (numpy.ones(n_bins) if e is None else e)

    def fit_triples(self, triples, resolution, n_bins, KRnorm=None, KRexpected=None, init=None,
                    complete=None, balance=None):
        """Solve straight from a Rao-format sparse file's content, never building
        the dense matrix: `triples` is the (n, 3) array [pos_i, pos_j, count] that
        `ContactMap.__init__` reads (reference `blueberry/datatypes.pyx:100-102`),
        bins are `int(pos / resolution)` (pyx:111-112), the matrix has
        `n_bins + 1` bins (pyx:97), and with KRnorm / KRexpected each count is
        balanced and O/E-normalised on the device as `ContactMap.normalize`
        would (pyx:166-169).  A bin pair that occurs more than once keeps its last
        count, as in the reference's scatter (pyx:115-116).
        complete='shortest_path' (see `fit`): the triples are scattered into a dense resident
        matrix (`ContactMap.from_triples`), normalised there if KR vectors are given, and that
        map is completed and fitted.
        balance: None, True or a dict of `balance_triples`' arguments (ignore_diags, min_nnz,
        tol, max_iter, row_sum, expected=False): the raw map is balanced first, on the device
        and from the very triples the fit reads (docs/SPEC.md 2.5.3), and the fit is that of
        `fit_triples(KRnorm=bias, KRexpected=ones)` -- with expected=True `KRexpected=e` -- bit
        for bit.  Leaves `bias_`, `balance_masked_`, `balance_iterations_`,
        `balance_converged_` and (expected=True) `expected_`.  It takes the place of KRnorm /
        KRexpected; with several devices the first one balances, in a distributed job every
        rank its own copy (the same bits); with complete='shortest_path' the dense map is
        balanced (`ContactMap.balance`).  `triples` may be a `DeviceTriples` on this solver's
        device (one-device fits without `complete`), which stays open."""
        _check_complete(complete)
        self._check_auto_route(complete)
        n = int(n_bins) + 1
        landmark = self._landmark_wanted(init)
        if landmark:
            self._check_landmark_route(complete)
        if balance is not None:
            if KRnorm is not None or KRexpected is not None:
                raise ValueError("balance= computes the bias itself: it takes no KRnorm / KRexpected")
            bal_args, bal_expected = _balance_options(balance)
            if not isinstance(triples, DeviceTriples):
                _check_triples(triples)
            if complete is None and not hasattr(self._engine_factory, "set_wish_triples"):
                raise ValueError("balance= runs on the device: this solver's engine has none")
        if KRnorm is not None and (numpy.any(numpy.asarray(KRnorm) == 0.0)
                                   or numpy.any(numpy.asarray(KRexpected)[:n_bins] == 0.0)):
            raise ZeroDivisionError("float division")      # as ContactMap.normalize
        if complete is not None:
            from .datatypes import ContactMap
            cm = ContactMap.from_triples(triples, resolution, n_bins, KRnorm=KRnorm,
                                         KRexpected=KRexpected, device=self._completion_device())
            if balance is not None:
                cm._KRnorm, cm._KRexpected = self._balance_on(cm, int(n_bins), bal_args, bal_expected)
            if KRnorm is not None or KRexpected is not None or balance is not None:
                cm.normalize()
            return self.fit(cm, init=init, complete=complete)
        if hasattr(self._engine_factory, "set_wish_triples"):
            # nan_to_num (pyx:102), the binning and the tile occupancy on the device: the host
            # never makes a pass over the triples (round 3: two isfinite passes, two divide +
            # astype passes and a scipy COO over 240 MB at chr1@10kb)
            devices = self._group_devices()
            if not (devices and len(devices) > 1):
                devices = [self._pick_device(_dist_state(self.distributed)[1])]
            # (several devices: every member packs from its own device's copy)
            with _resident_triples(triples, resolution, devices) as dev:
                try:
                    if balance is not None:
                        KRnorm, KRexpected = self._balance_on(dev, int(n_bins), bal_args, bal_expected)
                    if landmark:
                        start = self._landmark_init(dev, int(n_bins), KRnorm, KRexpected)
                        init = start if init is None else init
                    return self._fit_impl(dev, n, init, KRnorm, KRexpected)
                finally:
                    self._drop_anchor()
        # engines without a device (tests): bin on the host, as round 3 did
        t = _nan_to_num(_check_triples(triples))     # pyx:102 (no copy when every value is finite)
        rows = (t[:, 0] / resolution).astype(numpy.int64)
        cols = (t[:, 1] / resolution).astype(numpy.int64)
        import scipy.sparse
        keep = rows != cols
        sp = scipy.sparse.coo_matrix((t[keep, 2], (rows[keep], cols[keep])), shape=(n, n))
        return self._fit_impl(sp, n, init, KRnorm, KRexpected)

    def fit_many(self, maps, inits=None, complete=None):
        """Solve SEVERAL maps at once on one GPU -- e.g. the 23 per-chromosome ContactMaps
        of a genome (the reference's ContactMap is per chromosome, `blueberry/
        datatypes.pyx:88`), each of which alone is launch-bound (5-20 us per iteration
        whatever its size).  The maps are laid end to end in one blocked-sparse solver
        (`bb_solver_set_maps`): one sweep and one reduce launch per iteration serve all of
        them, every map with its own step (`lr='auto'`: 1 / (2 n_m)) and its own stress
        history.  Same iteration as `fit()` map by map; results agree with the single fits
        to rounding (1e-5 fp32 / 1e-12 fp64: the partial sums are cut differently), not bit
        for bit.  Inside a torch.distributed job the maps are dealt to the ranks by size,
        every rank solves its own in one solver on its GPU, and every rank gets all results
        (`ranks_of_maps_` tells who solved what): no exchange during the iterations.

        maps: sequence of ContactMaps (resident ones are packed device to device), square
        ndarrays or anything `numpy.asarray` takes.  inits: None, or one (n_m, 3) start per
        map (None entries: the seeded default of `fit()`).  complete='shortest_path' (see
        `fit`): every map is completed on the device that solves it and the fit is that of the
        completed maps under kind='wish'; `completed_unreachable_pairs_` is then a list.
        Sets `structures_` (list of (n_m, 3) float64), `stresses_` (list of per-iteration
        arrays), `n_bins_many_`, `lrs_`, `n_iter_`; returns self."""
        if self._group is not None and len(self._group) > 1:
            raise ValueError("fit_many with devices= / n_gpus= is not supported: fit_many runs "
                             "on one device, or one per rank of a torch.distributed job")
        _check_complete(complete)
        if self.alpha_auto:
            raise self._auto_refusal("is not for fit_many: its maps share one solver and one "
                                     "exponent, and a per-map alpha is not covered")
        if self.n_landmarks is not None:
            raise self._landmark_refusal("is not for fit_many, which packs dense blocks",
                                         "complete='shortest_path' or init='spectral'")
        if not hasattr(self._engine_factory, "set_maps"):
            raise TypeError("fit_many needs an engine that holds several maps (HipEngine)")
        maps = list(maps)
        if not maps:
            raise ValueError("fit_many needs at least one map")
        if inits is None:
            inits = [None] * len(maps)
        if len(inits) != len(maps):
            raise ValueError("inits needs one entry per map")
        rank, world = _dist_state(self.distributed)
        if world > 1:
            # Several GPUs: the maps are independent problems, so every rank solves maps of its
            # own (dealt by size, largest first, to the rank with the least pairs so far) and
            # the results are gathered -- no exchange during the iterations at all.
            import torch.distributed as dist
            sizes = [self._map_source(X, sparse=False)[1] for X in maps]
            load, mine = [0] * world, [[] for _ in range(world)]
            for m in sorted(range(len(maps)), key=lambda q: (-sizes[q], q)):
                r = min(range(world), key=lambda q: (load[q], q))
                load[r] += sizes[m] * sizes[m]
                mine[r].append(m)
            part = None
            if mine[rank]:
                local = self._clone(device=self._pick_device(world), distributed=False,
                                    devices=None, n_gpus=None)
                local._fit_many_local([maps[m] for m in mine[rank]], [inits[m] for m in mine[rank]],
                                      complete)
                part = (mine[rank], local.structures_, local.stresses_, local.lrs_,
                        getattr(local, "completed_unreachable_pairs_", None))
            parts = [None] * world
            dist.all_gather_object(parts, part)
            n = len(maps)
            self.structures_, self.stresses_, self.lrs_ = [None] * n, [None] * n, [None] * n
            unreachable = [None] * n
            for p in parts:
                if p is not None:
                    for k, m in enumerate(p[0]):
                        self.structures_[m], self.stresses_[m], self.lrs_[m] = p[1][k], p[2][k], p[3][k]
                        if p[4] is not None:
                            unreachable[m] = p[4][k]
            if complete is not None:
                self.completed_unreachable_pairs_ = unreachable
            self.n_bins_many_ = sizes
            self.n_iter_ = max(int(h.shape[0]) for h in self.stresses_)
            self.ranks_of_maps_ = [next(r for r in range(world) if m in mine[r]) for m in range(n)]
            return self
        return self._fit_many_local(maps, inits, complete)

    def _fit_many_local(self, maps, inits, complete=None):
        """fit_many on this rank's GPU (see fit_many)."""
        kind = self.kind
        if complete is not None:
            maps = [self._completed(X, device=self._pick_device(1)) for X in maps]
            self.completed_unreachable_pairs_ = [cm.unreachable_pairs_ for cm in maps]
            kind = "wish"
        pairs = [self._map_source(X, sparse=False) for X in maps]
        srcs, sizes = [src for src, _ in pairs], [n for _, n in pairs]
        if min(sizes) < 2:
            raise ValueError("every map needs at least 2 bins")
        # the tile edge of the joint layout: 128 only for a small fp64 problem
        def layout(vw):
            off = [0]
            for n in sizes[:-1]:
                off.append(off[-1] + -(-n // vw) * vw)
            return off, off[-1] + sizes[-1]
        off, total = layout(128)
        if layout_info(total, self.dtype)["vw"] != 128:
            off, total = layout(512)
        vw = layout_info(total, self.dtype)["vw"]
        ti, tj = [], []
        for o, n in zip(off, sizes):
            b0, b1 = o // vw, (o + n + vw - 1) // vw
            jj, ii = numpy.meshgrid(numpy.arange(b0, b1), numpy.arange(b0, b1))
            sel = ii <= jj
            ti.append(ii[sel])
            tj.append(jj[sel])
        ti, tj = numpy.concatenate(ti), numpy.concatenate(tj)
        order = numpy.lexsort((ti, tj))
        tiles = (ti[order].astype(numpy.int32), tj[order].astype(numpy.int32))
        lrs = [self._one_step(n) for n in sizes]
        device = self._pick_device(1)
        x0 = numpy.zeros((total, 3))
        for m, (o, n) in enumerate(zip(off, sizes)):
            init = inits[m]
            if init is None and self.init == "spectral":
                # each map's classical-MDS start from a solver of its own (device form), which
                # only makes the start: unweighted, one step for all, no iterations
                init = self._clone(n_iter=0, init="spectral", device=device, distributed=False,
                                   devices=None, n_gpus=None, degree_steps=False, weight_power=0,
                                   momentum=0.0, tol=None, kind=kind).fit(maps[m]).structure_
            elif init is None:
                init = self._default_start(n)
            x0[o:o + n] = _check_coords(init, n)
        eng = self._engine_factory(total, self.dtype, rank=0, world=1, device=device, tiles=tiles)
        with _teardown(eng):
            eng.set_maps(off + [total], lrs)
            for o, n, src in zip(off, sizes, srcs):
                if getattr(src, "is_resident", False) and src._resident().device == eng.device:
                    eng.set_wish_from_cm_block(src._resident(), o, kind, self.alpha)
                else:
                    m = src.to_host() if getattr(src, "is_resident", False) else src
                    eng.set_wish_dense_block(m, o, kind, self.alpha)
            sums = self._bin_sums(eng, 1)
            if sums is not None:
                # SPEC 2.3.1 / 2.4.1 per map: every bin's whole step goes into `steps`
                # (lr = 1 below), each map's `lr` -- 'auto' or a float -- being the step of its
                # best-connected bin
                steps = numpy.ones(total)
                for q, (o, n) in enumerate(zip(off, sizes)):
                    part = sums[o:o + n]
                    lrs[q], scale = self._steps(part, n)
                    if self.weight_power:
                        steps[o:o + n] = lrs[q] if scale is None else lrs[q] * scale
                    else:
                        # multiplied before it is divided: not the bits of lr * scale, the
                        # factors fit() hands to set_bin_steps (`degree_step_factors`)
                        steps[o:o + n] = lrs[q] * (part.max() + 1.0) / (part + 1.0)
                eng.set_bin_steps(steps)
            eng.set_coords(x0)
            if self.momentum:
                eng.set_momentum(self.momentum)
            nm = len(sizes)
            # converged: every map's last step decreased its stress by <= tol, relatively (a
            # map at stress 0 counts as converged, which the single fit() never stops on)
            self._iterate(lambda k: eng.iterate(k, 1.0),
                          lambda: eng.stress_history().reshape(-1, nm),
                          lambda h: h.shape[0] >= 2 and numpy.all(
                              numpy.abs(h[-2] - h[-1]) <= self.tol * numpy.maximum(h[-2], 1e-300)))
            X = eng.get_coords()
            hist = eng.stress_history().reshape(-1, nm)
        self.structures_ = [X[o:o + n].copy() for o, n in zip(off, sizes)]
        self.stresses_ = [hist[:, m].copy() for m in range(nm)]
        self.n_bins_many_, self.lrs_, self.n_iter_ = sizes, lrs, int(hist.shape[0])
        return self

    def fit_transform(self, X, init=None):
        """`fit(X)` and return the (n_bins, 3) coordinates."""
        return self.fit(X, init=init).structure_


def spectral_init(eng, n, world, n_iter=40, seed=0, tol=0.0, return_iterations=False):
    """Classical-MDS start: the top three eigenpairs of B = -1/2 J (D o D) J,
    J = I - 11'/n, by block power iteration with a Rayleigh-Ritz step, using the
    device matvec over the resident units (`bb_solver_matvec_sq`); X0 = V sqrt(L).
    This is the host-driven form (several ranks: the per-rank products are summed over
    the ranks between steps; and engines without a device); on one rank
    `HipEngine.spectral_init_device` runs the same iteration without leaving the device.
    Exact (up to a rigid motion) for a complete, noise-free distance matrix; for
    incomplete maps the missing pairs count as zero distance, so it is a start,
    not a solution.  tol > 0: the stopping rule of `bb_solver_spectral_init_tol` (after every
    product but the first, ||Z - V V'Z||_F / ||Z||_F < tol ends the loop).  Plays the part
    SURVEY.md 8(f)-2 assigns to the reference's `ContactMap.eigenvector`
    (`blueberry/datatypes.pyx:216-235`)."""
    def apply_B(V):
        U = V - V.mean(axis=0)
        W = _sum_over_ranks(eng.matvec_sq(U), eng, world)
        return -0.5 * (W - W.mean(axis=0))

    def orth(A):
        # fewer than 3 bins: QR gives fewer than 3 columns; the missing ones are zero directions
        Q = numpy.linalg.qr(A)[0]
        if Q.shape[1] < 3:
            Q = numpy.hstack([Q, numpy.zeros((n, 3 - Q.shape[1]))])
        return Q

    G0 = numpy.random.default_rng(seed).standard_normal((n, 3))
    V = orth(G0)
    done, Z = 0, None
    for it in range(int(n_iter)):
        Z = apply_B(V)
        if tol > 0.0 and it > 0:
            zz, G = float((Z * Z).sum()), V.T @ Z
            if (numpy.sqrt(max(0.0, zz - float((G * G).sum())) / zz) if zz > 0.0 else 0.0) < tol:
                break
        V, Z = orth(Z), None
        done = it + 1
    if Z is None:
        Z = apply_B(V)
    evals, evecs = numpy.linalg.eigh(0.5 * (V.T @ Z + Z.T @ V))       # Rayleigh-Ritz, 3x3
    order = numpy.argsort(evals)[::-1]
    U = V @ evecs[:, order]
    # an eigenvector's sign is arbitrary (numpy's eigh and the device path's Jacobi sweeps
    # need not agree): every Ritz vector is turned to the side of the start's first column,
    # here and in bb_solver_spectral_init, so one seed gives one start on every world size
    U = U * numpy.where(U.T @ G0[:, 0] < 0.0, -1.0, 1.0)
    x0 = U * numpy.sqrt(numpy.maximum(evals[order], 0.0))
    return (x0, done) if return_iterations else x0


def _all_ranks(ok):
    """Collective AND over the ranks of one local outcome: every rank learns whether
    ALL of them succeeded, so that all of them take the same next step."""
    import torch.distributed as dist
    flags = [None] * dist.get_world_size()
    dist.all_gather_object(flags, bool(ok))
    return all(flags)


_TRIAL_PEER_TIMEOUT_MS = 2000
_TRIAL_SYNC_TIMEOUT_MS = int(os.environ.get("BB_TRIAL_SYNC_TIMEOUT_MS", "30000"))


def _trial_leg(eng, name, step, lr, x0, iters):
    """One transport's trial run from the start x0: one step (coordinates kept for the
    agreement check), ten more to warm up, `iters` timed.  After EVERY stage the ranks
    agree on whether all of them got through it; the first stage that failed anywhere
    ends the leg on every rank, so nobody enters a collective that a peer has left.
    Returns (ok, coordinates after one step, seconds per iteration)."""
    import time
    import torch.distributed as dist
    box = {}

    def stage(fn):
        try:
            fn()
            ok = True
        except Exception as exc:                 # this transport is just not used
            eng._comm_trial_error = "%s: %s" % (name, exc)
            ok = False
        return _all_ranks(ok)

    def settle():
        # bounded: a collective that a peer never joined must end the leg, not the job
        bounded = getattr(eng, "sync_timeout", None)
        if bounded:
            bounded(_TRIAL_SYNC_TIMEOUT_MS)
        else:
            eng.sync()
        if name == "peer":
            eng.peer_status()                    # raises when a wait ran into its limit

    def first():
        eng.set_coords(x0)
        step(1, lr)
        settle()
        box["x1"] = eng.get_coords()

    def warm():
        step(10, lr)
        settle()

    def timed():
        t0 = time.perf_counter()
        step(iters, lr)
        settle()
        box["dt"] = (time.perf_counter() - t0) / iters
        box["xk"] = eng.get_coords()             # after 1 + 10 + iters steps (outside the clock)

    for k, fn in enumerate((first, warm, timed)):
        if k == 2:
            dist.barrier()
        if not stage(fn):
            return False, None, float("inf")
    # coordinates after the FIRST step and after the LAST: a transport that delivers a stale
    # or torn partial now and then shows in the second even when the first step went well
    return True, (box["x1"], box["xk"]), box["dt"]


def comm_reuse(eng):
    """Borrow the communicator an earlier solver of this job made: the library keeps one
    per (device, rank, world) for the life of the process, so only the first multi-rank
    fit() pays ncclCommInitRank (0.1-1 s; round 2 made and destroyed one per fit).
    Collective, and the same on every rank by construction: the ranks first agree that
    EVERY one of them holds a free cached communicator, then that every attach worked;
    otherwise nobody uses the cache and `comm_setup` makes a fresh one everywhere."""
    if hasattr(eng, "_comm_generation"):
        # ... and that it is the SAME communicator on all of them: the cache is keyed by
        # (device, rank, world) only, and a rank can hold one of another generation -- made
        # while a peer's earlier solver still held the previous one, or by an earlier process
        # group of the same size.  Attaching those would hang the first all-reduce.
        import torch.distributed as dist
        gens = [None] * dist.get_world_size()
        dist.all_gather_object(gens, eng._comm_generation())
        if gens[0] == 0 or any(g != gens[0] for g in gens):
            return False
    elif not _all_ranks(eng._comm_cached()):
        return False
    ok = eng._comm_attach()
    if not _all_ranks(ok):
        if ok:
            eng._comm_detach()
        return False
    return True


def _comm_get(eng):
    """The library's communicator for this engine: the one an earlier fit() of this job
    left in the library's cache (`comm_reuse`), else a new one (`comm_setup`).  Collective."""
    if hasattr(eng, "_comm_cached") and comm_reuse(eng):
        return True
    return eng.comm_setup()


def _exchange_state(eng):
    """The transport `select_exchange` chose for this engine ('group' for a GroupEngine), or
    None: nothing chosen yet, or an engine that never sums over ranks."""
    return getattr(eng, "_comm_state", None)


def select_exchange(eng, lr, trial=False):
    """Decide, once per engine and identically on every rank, how the partial
    gradients are summed over the ranks.  Collective.

    BB_COMM = auto (default) | peer | rccl | torch | host
      peer   one-shot exchange inside the solver's own kernels (IPC-mapped arenas)
      rccl   the library's own RCCL communicator, all-reduce enqueued from C
      torch  torch.distributed all-reduce on a tensor aliasing the exchange buffer
      host   exchange buffer staged through host memory (gloo / CPU rehearsals)
    auto on an RCCL job means rccl (torch if the communicator cannot be made).  With
    `trial` true -- bench.py, or BB_COMM_TRIAL=1 -- and the coordinates just set, auto
    also sets up peer and runs a few iterations through both from the same start
    (`_exchange_trial`).  The outcome is kept in eng._comm_state / eng._comm_trial."""
    if _exchange_state(eng):
        return eng._comm_state
    want = os.environ.get("BB_COMM", "auto")
    if want not in ("auto", "peer", "rccl", "torch", "host"):
        raise ValueError("BB_COMM must be auto, peer, rccl, torch or host, not %r" % want)
    trial = bool(trial) or os.environ.get("BB_COMM_TRIAL") == "1"
    state = _exchange_untried(eng, want, trial)
    if state is None:
        have_rccl = _comm_get(eng)
        if eng.peer_setup() and (have_rccl or hasattr(eng, "exchange_tensor")):
            state = _exchange_trial(eng, lr, have_rccl)
        else:
            state = "rccl" if have_rccl else "torch"
    eng._comm_state = state
    return state


def _exchange_untried(eng, want, trial):
    """The transport where no trial decides it, or None where one does (auto on an RCCL job
    with `trial`)."""
    import torch.distributed as dist
    native = hasattr(eng, "peer_setup")
    nccl = dist.get_backend() == "nccl"
    if not native or want == "host" or (not nccl and want != "peer"):
        return "host"
    if want == "peer":
        if not eng.peer_setup():
            raise RuntimeError("BB_COMM=peer but the peer exchange could not be set up: %s"
                               % eng._peer_error)
        # No trial has compared this exchange with RCCL: keep the two-launch form, which
        # applies a step whole or not at all and whose flags are ordered by release / acquire.
        # The one-launch form (data as its own flag, no fences) is taken where a trial has
        # validated it against RCCL on this very job, or on request (BB_PEER_FUSED=1).
        if not trial and os.environ.get("BB_PEER_FUSED") is None and hasattr(eng, "peer_set_form"):
            eng.peer_set_form(False)
        return "peer"
    if want == "torch":
        return "torch"
    if want == "rccl" or not trial:
        return "rccl" if _comm_get(eng) else "torch"
    return None


def _exchange_trial(eng, lr, have_rccl):
    """Run the peer exchange against a reference from the same start and return the one to
    use: peer only if its coordinates agree with the reference's and it is faster on the
    slowest rank; the start is restored afterwards.  The reference, which also runs if peer
    loses, is the library's communicator or -- when that could not be made --
    torch.distributed's all-reduce on the exchange buffer.  Every stage ends with an
    agreement between the ranks (`_trial_leg`), and the peer waits are cut to 2 s while it
    runs, so a transport that fails on one rank is dropped by all of them instead of leaving
    the others inside a collective.  Collective; the figures go to eng._comm_trial."""
    import torch.distributed as dist
    ref = "rccl" if have_rccl else "torch"
    ref_step = _stepper(eng, ref)
    x0 = eng.get_coords()
    set_limit = getattr(eng, "peer_set_timeout", None)
    if set_limit:
        set_limit(_TRIAL_PEER_TIMEOUT_MS)
    eng._comm_trial_error = None

    def reference_leg():
        run = _trial_leg(eng, ref, ref_step, lr, x0, 30)
        if have_rccl and not run[0] and hasattr(eng, "comm_abort"):
            # the library's communicator is suspect (this rank may still sit in a
            # collective a peer never joined): abort it -- every rank does,
            # the leg's outcome is shared -- so that the stream drains again
            try:
                eng.comm_abort()
            except Exception as exc:
                eng._comm_trial_error = "%s; abort: %s" % (eng._comm_trial_error, exc)
        return run

    runs = {"reference": reference_leg()}
    runs["peer"] = _trial_leg(eng, "peer", eng.iterate_peer, lr, x0, 30)
    if runs["reference"][0] and runs["peer"][0]:
        # the leg that runs first is timed on a chip whose clocks have not settled
        # (a block right after idle runs 4-19 % slow): the reference gets a
        # second timing behind the peer leg and keeps its better one.  (Leg outcomes
        # are agreed between the ranks, so every rank takes this branch or none.)
        again = reference_leg()
        if again[0]:
            runs["reference"] = (True, runs["reference"][1], min(runs["reference"][2], again[2]))
        else:
            runs["reference"] = again
    if set_limit and runs["peer"][0]:
        set_limit(int(os.environ.get("BB_PEER_TIMEOUT_MS", "10000")))
    eng.set_coords(x0)
    scale = float(numpy.abs(x0).max() + 1e-30)
    # one step: 1e-4 (the transports add the ranks' partials in different orders); the
    # whole leg, 41 steps: 1e-3 -- far above what the order of a sum does over that
    # many steps in fp32 (1e-5), far below what a lost or torn partial does
    agree = bool(runs["reference"][0] and runs["peer"][0]
                 and numpy.allclose(runs["reference"][1][0], runs["peer"][1][0], rtol=1e-4,
                                    atol=1e-6 * scale)
                 and numpy.allclose(runs["reference"][1][1], runs["peer"][1][1], rtol=1e-3,
                                    atol=1e-5 * scale))
    mine = (agree, runs["reference"][2], runs["peer"][2])
    every = [None] * eng.world
    dist.all_gather_object(every, mine)
    t_ref = max(e[1] for e in every)
    t_peer = max(e[2] for e in every)
    # the reference is the plain path: the peer exchange has to win by more than the
    # trial's own noise (3 %), not by a coin flip
    use_peer = all(e[0] for e in every) and t_peer < 0.97 * t_ref
    ms = lambda t: t * 1e3 if numpy.isfinite(t) else None
    eng._comm_trial = {"agree": all(e[0] for e in every), "reference": ref,
                       "rccl_ms": ms(t_ref),      # (the reference leg's time)
                       "peer_ms": ms(t_peer),
                       "error": eng._comm_trial_error}
    if use_peer:
        return "peer"
    return ref if runs["reference"][0] else "torch"


def _stepper(eng, state):
    """The callable (k, lr) that runs k iterations of `eng` with the transport `state`
    summing the ranks' partial gradients."""
    if state == "peer":
        return eng.iterate_peer
    if state == "rccl":
        return eng.iterate_dist

    def step(k, lr):
        # per iteration: local partial gradient -> sum over ranks -> identical update
        t = eng.exchange_tensor() if state == "torch" else None
        for _ in range(k):
            eng.grad()
            if t is None:
                allreduce_exchange_host(eng)
            else:
                allreduce_exchange(t)
            eng.apply(lr)
    return step


def run_iterations(eng, n_iter, lr, world):
    """n_iter solver iterations on an engine whose inputs are set.

    world == 1: the whole loop is enqueued by one C call.  world > 1: per
    iteration, local partial gradient -> sum over ranks -> identical update on
    every rank, so the replicas of X stay identical; `select_exchange` picks the
    transport."""
    if world == 1:
        eng.iterate(n_iter, lr)
    else:
        _stepper(eng, select_exchange(eng, lr))(n_iter, lr)
