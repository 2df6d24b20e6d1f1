"""The landmark constraints of docs/SPEC.md 2.5.5 in numpy float64, written from the specification
on top of tests/_landmark_model.py and independently of the package: nothing here imports
blueberry_amd.

  anchors_of   A[a][v] = the kept landmarks' geodesics rounded to the run's dtype by the value rule
               of every input route (tests/_input_model.flush_wish); 0 = no term: an unreachable
               node, a value outside the dtype's floor and ceiling, the landmark's own node
  objective    S(X) = S_q(X) + lambda sum_a sum_v A_av^-q (|x_{s_a} - x_v|_eps - A_av)^2 with its
               gradient: every ordered (a, v) is a term of its own and pulls on x_v and x_{s_a}
  sums_of      s_i = sum_j w_ij^-q (q = 0: the degree) + lambda sum over the terms touching i
  steps_of     lr = 1 / (2 max s), c_i = max s / s_i (1 where s_i = 0)       (SPEC 2.4.1)
  fit          K steps V <- mu V - lr c g, X <- X + V from X0; the history holds S before each step
The map is the symmetric matrix w of wish distances (0 = no constraint) of
tests/_landmark_model.weights_of; only its stored pairs i < j are visited."""
import numpy

from tests import _input_model as im
from tests import _landmark_model as lm

EPS2 = {"float32": 1e-30, "float64": 1e-300}                 # SPEC 2.2


def hic_like_triples(n, seed):
    """tests/test_gpu_landmark.py's generator, restated (that module imports the package): counts
    ~ Poisson(30 d^-3) on the persistent random walk chain_coords(n, seed), drawn by
    default_rng(100 + seed), as triples at resolution 1; the true pair distances; the random start
    drawn after the counts; the symmetric count matrix."""
    Xs = lm.chain_coords(n, seed)
    Ds = lm.pair_distances(Xs)
    r = numpy.random.default_rng(100 + seed)
    lam = 30.0 * numpy.maximum(Ds, 1e-9) ** -3.0
    numpy.fill_diagonal(lam, 0)
    C = numpy.triu(r.poisson(lam), 1).astype(float)
    X0 = r.standard_normal((n, 3))
    i, j = numpy.nonzero(C)
    return numpy.stack([i * 1.0, j * 1.0, C[i, j]], axis=1), Ds, X0, C + C.T


def anchors_of(g, landmarks, kept, dtype):
    """(A, nodes): the (L', n) float64 array of the kept rows of the geodesics g (+inf: no path)
    as a `dtype` run holds them, and the kept landmarks' nodes."""
    kept = numpy.asarray(kept, dtype=bool)
    nodes = numpy.asarray(landmarks, dtype=numpy.int64)[kept]
    A = im.flush_wish(lm.as_read(numpy.asarray(g)[kept]), dtype)
    A[numpy.arange(nodes.size), nodes] = 0.0
    return A, nodes


class Terms(object):
    """Every weighted term of the objective as flat arrays: (i, j, delta, factor), the stored
    pairs i < j with factor 1 and the landmark terms (s_a, v) with factor lambda."""

    def __init__(self, w, A, nodes, lam):
        w = numpy.asarray(w, dtype=numpy.float64)
        i, j = numpy.nonzero(numpy.triu(w, 1) > 0)
        self.n = w.shape[0]
        self.n_pairs = i.size
        if A is not None and lam > 0:
            a, v = numpy.nonzero(A > 0)
            self.i = numpy.concatenate([i, numpy.asarray(nodes)[a]])
            self.j = numpy.concatenate([j, v])
            self.delta = numpy.concatenate([w[i, j], A[a, v]])
            self.factor = numpy.concatenate([numpy.ones(i.size), numpy.full(a.size, float(lam))])
        else:
            self.i, self.j, self.delta, self.factor = i, j, w[i, j], numpy.ones(i.size)

    def weights(self, q):
        return self.factor * self.delta ** (-float(q)) if q else self.factor.copy()


def objective(X, terms, q, dtype="float64"):
    """(S, S_anchor, gradient) at X."""
    X = numpy.asarray(X, dtype=numpy.float64)
    diff = X[terms.i] - X[terms.j]
    d = numpy.sqrt((diff * diff).sum(axis=1) + EPS2[dtype])
    wt = terms.weights(q)
    res = d - terms.delta
    each = wt * res * res
    f = (2.0 * wt * res / d)[:, None] * diff
    g = numpy.zeros_like(X)
    for c in range(3):
        g[:, c] = (numpy.bincount(terms.i, weights=f[:, c], minlength=terms.n)
                   - numpy.bincount(terms.j, weights=f[:, c], minlength=terms.n))
    return float(each.sum()), float(each[terms.n_pairs:].sum()), g


def sums_of(terms, q):
    """(s, anchor part): the weighted degrees with the landmark terms, and the latter alone."""
    wt = terms.weights(q)
    both = lambda lo, hi: (numpy.bincount(terms.i[lo:hi], weights=wt[lo:hi], minlength=terms.n)
                           + numpy.bincount(terms.j[lo:hi], weights=wt[lo:hi], minlength=terms.n))
    anchor = both(terms.n_pairs, None)
    return both(0, terms.n_pairs) + anchor, anchor


def steps_of(s):
    """(lr, c) of SPEC 2.4.1 from the sums s."""
    top = float(s.max())
    return 1.0 / (2.0 * top), numpy.where(s > 0, top / numpy.where(s > 0, s, 1.0), 1.0)


def fit(X0, terms, q, n_iter, momentum=0.0, dtype="float64", every=None):
    """(history, anchor stress at the end, X, snapshots): n_iter steps from X0.  snapshots[k] = X
    after k steps for the k in `every`."""
    X = numpy.array(X0, dtype=numpy.float64)
    V = numpy.zeros_like(X)
    lr, c = steps_of(sums_of(terms, q)[0])
    history, shots = [], {}
    for k in range(int(n_iter)):
        S, _, g = objective(X, terms, q, dtype)
        history.append(S)
        V = momentum * V - lr * c[:, None] * g
        X = X + V
        if every and k + 1 in every:
            shots[k + 1] = X.copy()
    return numpy.array(history), objective(X, terms, q, dtype)[1], X, shots


def spearman(X, Ds):
    """Spearman correlation of the pair distances of X with the true ones Ds, pairs i < j."""
    import scipy.stats
    iu = numpy.triu_indices(Ds.shape[0], 1)
    return float(scipy.stats.spearmanr(lm.pair_distances(X[:Ds.shape[0]])[iu], Ds[iu])[0])


def fold_case(n, n_landmarks, seed=1, start_seed=0):
    """The map of the fold table: hic_like_triples(n, seed) over n nodes (fit_triples' n_bins =
    n - 1), counts, alpha = 3, its landmark start (default start seed `start_seed`) and float64
    anchors: (w, Ds, start, A, nodes)."""
    triples, Ds, _, _ = hic_like_triples(n, seed)
    w = lm.weights_of(triples, 1, n, kind="counts", alpha=3.0)
    start, landmarks, kept, _, _, _, g = lm.landmark_start_of(w, n_landmarks, start_seed)
    A, nodes = anchors_of(g, landmarks, kept, "float64")
    return w, Ds, start, A, nodes
