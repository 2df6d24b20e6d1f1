"""CPU: what the landmark start (docs/SPEC.md 2.1.2, 2.5.4) rests on, without a device -- the
fixed point of Bellman-Ford is Dijkstra's result bit for bit (the property
tests/test_gpu_landmark.py leans on), `landmark_coefficients` places embeddable point sets, its
sign and rank rules, the landmark choice, and every refusal that comes before a device is
touched."""
import numpy
import pytest

import blueberry_amd as bb
from blueberry_amd import solver as bs
from tests import _landmark_model as lm
from tests._engines import OracleEngine
from tests._util import bits


# ---- 1. the fixed point is Dijkstra's, bit for bit -------------------------------------------
@pytest.mark.parametrize("seed", range(12))
def test_bellman_ford_in_any_order_equals_dijkstra_bit_for_bit(seed):
    rng = numpy.random.default_rng(seed)
    n = int(rng.integers(5, 90))
    w = lm.weights_of(lm.random_graph_triples(n, int(rng.integers(n, 4 * n)), seed), 1, n, kind="wish")
    assert (w > 0).any()
    for source in rng.integers(0, n, 3):
        want = lm.geodesics(w, [source])[0]
        jac, s_jac = lm.bellman_ford_jacobi(w, int(source))
        inp, s_inp = lm.bellman_ford_in_place(w, int(source), rng)
        assert numpy.array_equal(bits(jac), bits(want))
        assert numpy.array_equal(bits(inp), bits(want))
        assert 1 <= s_inp <= s_jac <= n


# ---- 2. landmark_coefficients ------------------------------------------------------------------
def _points(kind, n, seed):
    if kind == "walk":
        return lm.chain_coords(n, seed)
    return numpy.random.default_rng(seed).standard_normal((n, 3)) * numpy.array([3.0, 2.0, 1.0])


@pytest.mark.parametrize("L", [4, 5, 16, 64])
@pytest.mark.parametrize("kind", ["random", "walk"])
def test_coefficients_place_embeddable_points_exactly(kind, L):
    """Euclidean distances in 3-D are exactly embeddable: landmark MDS reproduces every pair
    distance.  Bound 1e-10 of the largest distance (a numpy model measured 3.3e-13 as the worst
    of 20 configurations; the factor 300 covers another LAPACK)."""
    n = 200
    X = _points(kind, n, seed=L)
    D = lm.pair_distances(X)
    marks = lm.landmarks_of(range(n), L)
    coef, mu = bb.landmark_coefficients(D[numpy.ix_(marks, marks)])
    assert coef.shape == (L, 3) and mu.shape == (L,)
    Y, placed, _ = lm.place_of(D[marks], coef, mu)
    assert placed.all()
    err = numpy.abs(lm.pair_distances(Y) - D).max() / D.max()
    print("%s L=%d: worst pair-distance error %.3e of the largest distance" % (kind, L, err))
    assert err <= 1e-10
    # the independent model of the rule agrees to rounding
    coef_m, mu_m = lm.coefficients_of(D[numpy.ix_(marks, marks)])
    assert numpy.allclose(mu, mu_m, rtol=1e-13, atol=0)
    assert numpy.allclose(coef, coef_m, rtol=0, atol=1e-9 * numpy.abs(coef_m).max())


def test_sign_rule_and_zero_columns():
    rng = numpy.random.default_rng(3)
    X = rng.standard_normal((9, 3))
    coef, _ = bb.landmark_coefficients(lm.pair_distances(X))
    for c in range(3):
        big = int(numpy.argmax(numpy.abs(coef[:, c])))
        assert coef[big, c] > 0
    # mirrored points: the same coefficients (distances do not see the mirror)
    coef2, _ = bb.landmark_coefficients(lm.pair_distances(-X))
    assert numpy.array_equal(coef, coef2)
    # collinear points: one direction, two zero columns; coplanar: one zero column
    line = numpy.arange(7.0)[:, None] * numpy.array([1.0, 2.0, 2.0])
    coef, mu = bb.landmark_coefficients(lm.pair_distances(line))
    assert numpy.any(coef[:, 0] != 0) and not coef[:, 1:].any()
    Y, _, _ = lm.place_of(lm.pair_distances(line), coef, mu)
    assert numpy.allclose(lm.pair_distances(Y), lm.pair_distances(line), atol=1e-10 * 18)
    plane = numpy.concatenate([rng.standard_normal((8, 2)), numpy.zeros((8, 1))], axis=1)
    coef, _ = bb.landmark_coefficients(lm.pair_distances(plane))
    assert numpy.any(coef[:, 1] != 0) and not coef[:, 2].any()
    # all landmarks in one place: nothing to place by
    coef, mu = bb.landmark_coefficients(numpy.zeros((5, 5)))
    assert not coef.any() and not mu.any()
    # an asymmetric input is symmetrised through its squares
    G = lm.pair_distances(X)
    A = G.copy()
    A[0, 1], A[1, 0] = G[0, 1] * 1.5, G[0, 1] * 0.5
    S = G.copy()
    S[0, 1] = S[1, 0] = numpy.sqrt(0.5 * (A[0, 1] ** 2 + A[1, 0] ** 2))
    assert numpy.allclose(bb.landmark_coefficients(A)[0], bb.landmark_coefficients(S)[0], atol=1e-12)
    with pytest.raises(ValueError):
        bb.landmark_coefficients(numpy.zeros((3, 4)))


# ---- 3. the choice of landmarks ------------------------------------------------------------------
def test_landmark_choice_on_live_sets_with_gaps():
    live = numpy.array([2, 3, 5, 8, 13, 21, 34, 55, 89, 144])
    assert list(bs.landmark_choice(live, 4)) == [3, 8, 34, 89]          # indices 1, 3, 6, 8
    assert list(bs.landmark_choice(live, 10)) == list(live)
    assert list(bs.landmark_choice(live, 64)) == list(live)             # never more than live
    assert list(bs.landmark_choice(live[:3], 4)) == [2, 3, 5]
    assert bs.landmark_choice(numpy.array([], dtype=numpy.int64), 8).size == 0
    rng = numpy.random.default_rng(0)
    for _ in range(30):
        n = int(rng.integers(1, 400))
        live = numpy.flatnonzero(rng.random(n) < 0.6)
        L = int(rng.integers(4, 80))
        got = bs.landmark_choice(live, L)
        assert numpy.array_equal(got, lm.landmarks_of(live, L)) if live.size else got.size == 0
        assert numpy.all(numpy.diff(got) > 0) and numpy.isin(got, live).all()


# ---- 4. refusals before a device is touched -----------------------------------------------------
@pytest.mark.parametrize("bad", [("landmark", 3), ("landmark", 1025), ("landmark", 16.0),
                                 ("landmark", True), ("landmark", "16"), ("landmark",),
                                 ("spectral", 16), "landmarks", None, ["landmark", 16]])
def test_constructor_refuses_a_bad_landmark_init(bad):
    with pytest.raises(ValueError, match="landmark"):
        bb.StructureSolver(init=bad)


def test_constructor_takes_the_landmark_init_and_clones_carry_it():
    assert bb.StructureSolver(init="landmark").n_landmarks == 64
    s = bb.StructureSolver(init=("landmark", 16), seed=5)
    assert s.n_landmarks == 16 and s._clone().n_landmarks == 16 and s._clone().init == ("landmark", 16)
    assert bb.StructureSolver(init=("landmark", 4)).n_landmarks == 4
    assert bb.StructureSolver(init=("landmark", 1024)).n_landmarks == 1024
    assert bb.StructureSolver().n_landmarks is None
    assert bb.StructureSolver(init="spectral").n_landmarks is None


def test_fit_refusals_name_the_alternative():
    import scipy.sparse
    dense = numpy.ones((6, 6)) - numpy.eye(6)
    sparse = scipy.sparse.coo_matrix(dense)
    triples = numpy.array([[0.0, 1.0, 2.0], [1.0, 2.0, 2.0]])
    s = bb.StructureSolver(init="landmark", n_iter=1)
    for X in (dense, bb.ContactMap.from_matrix(dense), dense.tolist()):
        with pytest.raises(ValueError, match=r"complete='shortest_path' or init='spectral'"):
            s.fit(X)
    with pytest.raises(ValueError, match=r"complete='shortest_path'"):
        s.fit(dense, complete="shortest_path")
    with pytest.raises(ValueError, match=r"init='landmark' does not go with complete"):
        s.fit(sparse, complete="shortest_path")
    with pytest.raises(ValueError, match=r"init='landmark' does not go with complete"):
        s.fit_triples(triples, 1, 5, complete="shortest_path")
    with pytest.raises(ValueError, match=r"fit_many.*complete='shortest_path' or init='spectral'"):
        s.fit_many([dense, dense])
    with pytest.raises(ValueError, match=r"fit_many"):
        s.fit_many([dense], inits=[numpy.zeros((6, 3))])
    # an engine without a device
    host = bb.StructureSolver(init=("landmark", 8), n_iter=1, engine=OracleEngine)
    with pytest.raises(ValueError, match=r"engine has none; use init='spectral'"):
        host.fit_triples(triples, 1, 5)
    with pytest.raises(ValueError, match=r"engine has none; use init='spectral'"):
        host.fit(sparse)
    # landmark_start's own arguments
    for n_landmarks in (3, 1025, 8.0, True):
        with pytest.raises(ValueError, match="n_landmarks"):
            bb.landmark_start(triples, 1, 5, n_landmarks=n_landmarks)
    with pytest.raises(ValueError, match="resolution"):
        bb.landmark_start(triples, 0, 5)
    with pytest.raises(ValueError, match="shape"):
        bb.landmark_start(numpy.zeros((3, 2)), 1, 5)


def test_an_explicit_start_overrides_the_landmark_init(oracle):
    """init= given to fit() wins, as with every other start: the fit of a dense map under an
    engine without a device runs as it always did."""
    dense = numpy.ones((6, 6)) - numpy.eye(6)
    x0 = numpy.random.default_rng(1).standard_normal((6, 3))
    kw = dict(n_iter=3, dtype="float64", kind="wish", engine=OracleEngine)
    got = bb.StructureSolver(init="landmark", **kw).fit(dense, init=x0)
    want = bb.StructureSolver(**kw).fit(dense, init=x0)
    assert numpy.array_equal(got.structure_, want.structure_)
