"""CPU: the numpy float64 model of the landmark constraints (docs/SPEC.md 2.5.5,
tests/_anchor_model.py) -- its gradient, its descent, the fold table the feature was proposed
with -- and the constructor refusals, which need no device."""
import numpy
import pytest

import blueberry_amd as bb
from tests import _anchor_model as am
from tests import _landmark_model as lm


def test_the_generator_is_the_landmark_tests_generator():
    from tests.test_gpu_landmark import hic_like_triples
    for a, b in zip(am.hic_like_triples(120, 3), hic_like_triples(120, 3)):
        assert numpy.array_equal(a, b)


@pytest.fixture(scope="module")
def chain400():
    return am.fold_case(400, 16)


def test_anchor_rows_follow_the_value_rule():
    g = numpy.array([[0.0, 1.5, numpy.inf, 1e-31, 1e39, 0.1],
                     [2.0, 0.0, 3.0, 1e-291, numpy.inf, 0.2],
                     [9.0, 9.0, 9.0, 9.0, 9.0, 9.0]])
    A32, nodes = am.anchors_of(g, [0, 1, 5], [True, True, False], "float32")
    assert numpy.array_equal(nodes, [0, 1])
    assert numpy.array_equal(A32, [[0, 1.5, 0, 0, 0, numpy.float32(0.1)], [2, 0, 3, 0, 0, numpy.float32(0.2)]])
    A64, _ = am.anchors_of(g, [0, 1, 5], [True, True, False], "float64")
    assert numpy.array_equal(A64, [[0, 1.5, 0, 1e-31, 1e39, 0.1], [2, 0, 3, 0, 0, 0.2]])


@pytest.mark.parametrize("q", [0, 1, 2])
def test_gradient_against_central_differences(q):
    n = 40
    triples, _, _, _ = am.hic_like_triples(n, 5)
    w = lm.weights_of(triples, 1, n, kind="counts", alpha=3.0)
    _, landmarks, kept, _, _, _, g = lm.landmark_start_of(w, 6, 0)
    A, nodes = am.anchors_of(g, landmarks, kept, "float64")
    terms = am.Terms(w, A, nodes, 0.7)
    # a landmark pair that is also a stored pair, and both orders of a landmark pair, are terms
    assert (A[:, nodes] > 0).sum() == nodes.size * (nodes.size - 1)
    X = numpy.random.default_rng(q).standard_normal((n, 3))
    S, Sa, grad = am.objective(X, terms, q)
    assert 0 < Sa < S
    h = 1e-6
    for i, c in [(0, 0), (int(nodes[0]), 1), (int(nodes[-1]), 2), (n - 1, 0), (17, 1)]:
        Xp, Xm = X.copy(), X.copy()
        Xp[i, c] += h
        Xm[i, c] -= h
        fd = (am.objective(Xp, terms, q)[0] - am.objective(Xm, terms, q)[0]) / (2 * h)
        assert abs(fd - grad[i, c]) <= 1e-6 * numpy.abs(grad).max()
    # lambda = 0 is the unanchored objective
    S0, Sa0, g0 = am.objective(X, am.Terms(w, A, nodes, 0.0), q)
    assert Sa0 == 0.0 and S0 < S and not numpy.array_equal(g0, grad)


@pytest.mark.parametrize("q", [0, 1, 2])
@pytest.mark.parametrize("lam", [0.1, 1.0, 10.0])
def test_the_anchored_steps_never_raise_the_stress(chain400, q, lam):
    """SPEC 2.4.1's Gershgorin argument with the weights {1, lambda, 1 + lambda} delta^-q: 200
    steps with a step per bin on hic_like_triples(400, 1), 16 landmarks."""
    w, _, start, A, nodes = chain400
    history, Sa, _, _ = am.fit(start, am.Terms(w, A, nodes, lam), q, 200)
    assert (numpy.diff(history) <= 0).all() and history[-1] < history[0] and Sa > 0


# The table of docs/SPEC.md 2.5.5: Spearman correlation of fitted and true pair distances after
# 100, 300 and 1000 steps.  Map: hic_like_triples(n, 1) (chain seed 1, counts drawn by
# default_rng(101)), counts, alpha = 3, n nodes; landmark start with the default start's seed 0.
FOLD_TABLE = {
    (1000, 32): (0.870, {(0.0, 0): (0.778, 0.731, 0.663), (0.1, 0): (0.835, 0.837, 0.840),
                         (1.0, 0): (0.838, 0.850, 0.855), (0.0, 2): (0.797, 0.755, 0.705),
                         (1.0, 2): (0.831, 0.820, 0.814)}),
    (400, 16): (0.956, {(0.0, 0): (0.957, 0.956, 0.948), (0.1, 0): (0.959, 0.959, 0.958)}),
}


@pytest.mark.parametrize("case", sorted(FOLD_TABLE))
def test_the_fold_table(case, chain400):
    n, L = case
    w, Ds, start, A, nodes = chain400 if n == 400 else am.fold_case(n, L)
    r_start, rows = FOLD_TABLE[case]
    assert abs(am.spearman(start, Ds) - r_start) < 5e-4
    for (lam, q), want in sorted(rows.items()):
        history, _, _, shots = am.fit(start, am.Terms(w, A, nodes, lam), q, 1000, every=(100, 300, 1000))
        got = tuple(am.spearman(shots[k], Ds) for k in (100, 300, 1000))
        print(case, "lambda %g q %d:" % (lam, q), " ".join("%.3f" % r for r in got),
              "stress %.0f -> %.0f" % (history[0], history[-1]))
        assert max(abs(a - b) for a, b in zip(got, want)) < 5e-4
        assert (numpy.diff(history) <= 0).all()


def test_constructor_refusals_need_no_device():
    ok = bb.StructureSolver(init=("landmark", 32, 0.1), degree_steps=True)
    assert ok.landmark_weight == 0.1 and ok.n_landmarks == 32
    assert ok._clone().landmark_weight == 0.1
    for init in ("random", "spectral", "landmark", ("landmark", 16), ("landmark", 16, 0.0), ("landmark", 16, 0)):
        assert bb.StructureSolver(init=init).landmark_weight == 0.0       # today's fits, no degree_steps needed
    with pytest.raises(ValueError, match="needs degree_steps=True.*slow every bin"):
        bb.StructureSolver(init=("landmark", 32, 0.1))
    for bad in (-0.1, float("nan"), float("inf"), "1", True, None):
        with pytest.raises(ValueError, match="landmark_weight must be a finite number >= 0"):
            bb.StructureSolver(init=("landmark", 32, bad), degree_steps=True)
    with pytest.raises(ValueError, match="init must be"):
        bb.StructureSolver(init=("spectral", 32, 0.1), degree_steps=True)   # (a weight goes with 'landmark' alone)
    with pytest.raises(ValueError, match="init must be"):
        bb.StructureSolver(init=("landmark", 32, 0.1, 1), degree_steps=True)
    for several in (dict(devices=[0, 1]), dict(n_gpus=2), dict(devices=[0, 0])):
        with pytest.raises(ValueError, match="init='landmark' with landmark_weight > 0 keeps its constraints "
                                             "on one device"):
            bb.StructureSolver(init=("landmark", 32, 0.1), degree_steps=True, **several)
        bb.StructureSolver(init=("landmark", 32), degree_steps=True, **several)     # the start alone may
    bb.StructureSolver(init=("landmark", 32, 0.1), degree_steps=True, devices=[0])


def test_route_refusals_need_no_device():
    import scipy.sparse
    from tests._engines import OracleEngine
    t = numpy.array([[0.0, 1.0, 2.0], [1.0, 2.0, 3.0]])
    s = bb.StructureSolver(init=("landmark", 4, 0.5), degree_steps=True)
    with pytest.raises(ValueError, match="init='landmark' does not go with complete='shortest_path'"):
        s.fit_triples(t, 1, 5, complete="shortest_path")
    with pytest.raises(ValueError, match="init='landmark' does not go with complete='shortest_path'"):
        s.fit(scipy.sparse.coo_matrix(numpy.eye(4)), complete="shortest_path")
    with pytest.raises(ValueError, match="init='landmark' is not for fit_many"):
        s.fit_many([numpy.ones((4, 4))])
    # an array as the call's init replaces the start only: the constraints still need the route
    with pytest.raises(ValueError, match="init='landmark' needs a sparse input"):
        s.fit(numpy.ones((6, 6)), init=numpy.zeros((6, 3)))
    e = bb.StructureSolver(init=("landmark", 4, 0.5), degree_steps=True, engine=OracleEngine, distributed=False)
    with pytest.raises(ValueError, match="init='landmark' runs on the device and this solver's engine has none"):
        e.fit_triples(t, 1, 5)
    with pytest.raises(ValueError, match="init='landmark' runs on the device and this solver's engine has none"):
        e.fit_triples(t, 1, 5, init=numpy.zeros((6, 3)))
