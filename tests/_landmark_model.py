"""The landmark start of docs/SPEC.md 2.1.2 / 2.5.4 in numpy and scipy float64, written from the
specification and independently of the package: the graph of a triple list, its geodesics, the
landmark rule and the placement sum.  No library code: nothing here imports blueberry_amd.

  weights    the rules of tests/_input_model.py for the 'triples' route in float64: nan_to_num,
             bin = trunc(pos / resolution), the LAST triple of an unordered pair wins, KR
             division then nan_to_num, wish_from_value; 0 = no edge; a bin outside the graph is
             a ValueError
  geodesics  scipy.sparse.csgraph.dijkstra(directed=False); +inf where there is no path
  landmarks  live = nodes with an edge, ascending; L = min(n_landmarks, len(live)); landmark k =
             live[((2 k + 1) len(live)) // (2 L)]
  placement  x_j = -1/2 sum_a coef[a] (D[a][j]^2 - mu[a]), a ascending
"""
import numpy

from tests import _input_model as im


def weights_of(triples, resolution, n_nodes, kind="counts", alpha=3.0, kr=None, ke=None):
    """The symmetric (n_nodes, n_nodes) float64 matrix of edge weights; 0 = no edge."""
    return im.matrix_of("triples", n_nodes, "float64", kind=kind, alpha=alpha, triples=triples,
                        resolution=resolution, kr=kr, ke=ke)


def edge_degrees_of(w):
    return im.degrees_of(w)


def geodesics(w, sources):
    """(len(sources), n) float64 shortest-path lengths over the weights w; +inf without a path."""
    import scipy.sparse
    import scipy.sparse.csgraph
    src = numpy.asarray(sources, dtype=numpy.int64)
    g = scipy.sparse.csgraph.dijkstra(scipy.sparse.csr_matrix(w), directed=False, indices=src)
    return numpy.asarray(g, dtype=numpy.float64).reshape(src.shape[0], w.shape[0])


def as_read(g):
    """Geodesics as the library hands them out: 0 where there is no path."""
    return numpy.where(numpy.isinf(g), 0.0, g)


def _adjacency(w):
    return [[(int(u), float(w[v, u])) for u in numpy.flatnonzero(w[v] > 0)] for v in range(w.shape[0])]


def bellman_ford_jacobi(w, source):
    """d[v] = min(d[v], fl(d[u] + w(u, v))) from the values of the sweep before, to the fixed
    point: (d, sweeps), the confirming sweep included."""
    n, adj = w.shape[0], _adjacency(w)
    d = [float("inf")] * n
    d[source] = 0.0
    for sweep in range(1, n + 1):
        new = list(d)
        for v in range(n):
            for u, wt in adj[v]:
                if d[u] + wt < new[v]:
                    new[v] = d[u] + wt
        if new == d:
            return numpy.array(d), sweep
        d = new
    raise AssertionError("no fixed point after n sweeps")


def bellman_ford_in_place(w, source, rng):
    """The same relaxation in place, the rows of every sweep in a random order."""
    n, adj = w.shape[0], _adjacency(w)
    d = [float("inf")] * n
    d[source] = 0.0
    for sweep in range(1, n + 1):
        changed = False
        for v in rng.permutation(n):
            for u, wt in adj[v]:
                if d[u] + wt < d[v]:
                    d[v] = d[u] + wt
                    changed = True
        if not changed:
            return numpy.array(d), sweep
    raise AssertionError("no fixed point after n sweeps")


def landmarks_of(live, n_landmarks):
    live = [int(v) for v in live]
    L = min(int(n_landmarks), len(live))
    return numpy.array([live[((2 * k + 1) * len(live)) // (2 * L)] for k in range(L)], dtype=numpy.int64)


def coefficients_of(G):
    """(coef, mu) by the rule of SPEC 2.5.4, with explicit loops where the package has none."""
    G = numpy.asarray(G, dtype=numpy.float64)
    L = G.shape[0]
    d2 = numpy.empty((L, L))
    for a in range(L):
        for b in range(L):
            d2[a, b] = 0.5 * (G[a, b] * G[a, b] + G[b, a] * G[b, a])
    mu = d2.mean(axis=0)
    J = numpy.eye(L) - numpy.full((L, L), 1.0 / L)
    lam, vec = numpy.linalg.eigh(-0.5 * (J @ d2 @ J))
    coef = numpy.zeros((L, 3))
    for c in range(min(3, L)):
        l_c, v = lam[L - 1 - c], vec[:, L - 1 - c].copy()
        if not (lam[L - 1] > 0 and l_c > 1e-12 * lam[L - 1]):
            continue
        big = max(range(L), key=lambda q: (abs(v[q]), -q))
        if v[big] < 0:
            v = -v
        coef[:, c] = v / numpy.sqrt(l_c)
    return coef, mu


def place_of(g, coef, mu):
    """(X, placed, bound) from the (L, n) geodesics g (+inf: no path): the placement sum over the
    sources that take part (a source whose coef row and mu are all 0 does not), a ascending;
    placed[j]: every one of them reaches j; bound (n, 3): 4 L 2^-53 sum_a |coef[a][c]| (g[a][j]^2 +
    |mu[a]|), what L fused or unfused multiply-adds may differ by."""
    L, n = g.shape
    part = [a for a in range(L) if numpy.any(coef[a] != 0.0) or mu[a] != 0.0]
    placed = numpy.ones(n, dtype=bool)
    X, mag = numpy.zeros((n, 3)), numpy.zeros((n, 3))
    for a in part:
        placed &= ~numpy.isinf(g[a])
    for a in part:
        d = numpy.where(placed, g[a], 0.0)
        X += coef[a][None, :] * (d * d - mu[a])[:, None]
        mag += numpy.abs(coef[a])[None, :] * (d * d + abs(mu[a]))[:, None]
    return -0.5 * X, placed, 4.0 * L * 2.0 ** -53 * mag


def landmark_start_of(w, n_landmarks, seed):
    """The whole rule on the weights w: (start, landmarks, kept, placed, coef, mu, g)."""
    n = w.shape[0]
    live = numpy.flatnonzero(edge_degrees_of(w) > 0)
    lm = landmarks_of(live, n_landmarks)
    g = geodesics(w, lm)
    reach = (~numpy.isinf(g)).sum(axis=1)
    main = int(numpy.argmax(reach))
    kept = ~numpy.isinf(g[main, lm])
    if kept.sum() < 4:
        raise ValueError("too disconnected")
    coef, mu = numpy.zeros((lm.size, 3)), numpy.zeros(lm.size)
    coef[kept], mu[kept] = coefficients_of(as_read(g[numpy.ix_(kept, lm[kept])]))
    X, placed, _ = place_of(g, coef, mu)
    start = numpy.random.default_rng(seed).standard_normal((n, 3))
    start[placed] = X[placed]
    return start, lm, kept, placed, coef, mu, g


# ---- generators ---------------------------------------------------------------------------------
def random_graph_triples(n, m, seed, resolution=1, wish=True):
    """m random triples over n nodes (diagonal ones among them) as [pos_i, pos_j, value]: real
    weights in (0.1, 2) for wish=True, else counts 4^-k, k in 0..5 -- with alpha = 1 their wish
    distance 4^k is exact in any pow()."""
    rng = numpy.random.default_rng(seed)
    i, j = rng.integers(0, n, m), rng.integers(0, n, m)
    v = rng.uniform(0.1, 2.0, m) if wish else 4.0 ** -rng.integers(0, 6, m).astype(numpy.float64)
    return numpy.stack([i * float(resolution), j * float(resolution), v], axis=1)


def chain_coords(n, seed):
    """The persistent random walk of tests/test_gpu_shortest_paths.py's fold test."""
    r = numpy.random.default_rng(seed)
    steps = r.standard_normal((n, 3))
    v = numpy.zeros(3)
    X = numpy.zeros((n, 3))
    for i in range(1, n):
        v = 0.8 * v + steps[i]
        X[i] = X[i - 1] + v / numpy.linalg.norm(v)
    return X


def pair_distances(X):
    d = X[:, None, :] - X[None, :, :]
    return numpy.sqrt((d * d).sum(axis=2))
