"""The landmark start for sparse maps (docs/SPEC.md 2.5.4): landmark MDS over shortest paths on
the stored pairs of device triples."""
import numpy

from .ranks import pick_device, several_ranks
from .triples import GeodesicRows, _bin_count, _resident_triples


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
    with _resident_triples(triples, resolution, [pick_device(device, several_ranks())]) as dev:
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
