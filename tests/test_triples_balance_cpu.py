"""CPU: the sparse model of docs/SPEC.md 2.5.3 (tests/_triples_model.py) against the dense model of
2.5.2 (tests/_balance_model.py) on the same maps given as triples, and the argument checks of
`balance_triples` / `fit_triples(balance=...)`, which must raise before the library is loaded.

The two models add a row's terms in different orders (a dense row with its zeros, a CSR row
without), so the bias and e agree to the bound of tests/test_gpu_balance.py -- one sum of at most
d non-negative terms on each side, the iteration contractive: (d + 16) 2^-52 relative -- while the
mask and the number of updates must be EQUAL.  Every toleranced figure is printed before it is
asserted (`pytest -s`)."""
import numpy
import pytest

import blueberry_amd as bb
from blueberry_amd import _lib
from tests import _balance_model as bm
from tests import _triples_model as tm
from tests._util import max_rel

SIZES = [2, 3, 64, 65, 66, 129, 1025]
BANDS = [0, 2, 17]
EPS = 2.0 ** -52


def maps(d):
    return [("hic", bm.hic_like_raw(d), 0), ("integer", bm.integer_map(d, d)[0], 5)]


@pytest.mark.parametrize("ignore_diags", BANDS)
@pytest.mark.parametrize("d", SIZES)
def test_the_sparse_model_is_the_dense_model(d, ignore_diags):
    n = d - 1
    bound = (d + 16) * EPS
    for name, m, min_nnz in maps(d):
        t = tm.triples_of_matrix(m)
        for tol, max_iter in ((0.0, 20), (1e-5, 200)):
            try:
                want = bm.balance(m, ignore_diags, min_nnz, tol, max_iter)
            except ValueError as err:
                assert "no live bin" in str(err)
                with pytest.raises(ValueError, match="no live bin"):
                    tm.balance(t, tm.RESOLUTION, n, ignore_diags, min_nnz, tol, max_iter)
                continue
            got = tm.balance(t, tm.RESOLUTION, n, ignore_diags, min_nnz, tol, max_iter)
            err = max_rel(got["bias"], want["bias"])
            print("%s d=%d band=%d tol=%g: %d updates (dense %d), bias error %.2e (bound %.2e)"
                  % (name, d, ignore_diags, tol, got["iterations"], want["iterations"], err, bound))
            assert numpy.array_equal(got["masked"], want["masked"])
            assert got["iterations"] == want["iterations"] and got["converged"] == want["converged"]
            assert err <= bound
            sums, counts, e = bm.expected(m, want["bias"])
            s2, c2, e2 = tm.expected(t, tm.RESOLUTION, n, want["bias"])
            err = max_rel(e2, e)
            print("   e error %.2e" % err)
            assert numpy.array_equal(c2, counts) and err <= bound
        sums, counts, e = bm.expected(m, None)
        s2, c2, e2 = tm.expected(t, tm.RESOLUTION, n, None)
        assert numpy.array_equal(c2, counts)
        if name == "integer":
            assert numpy.array_equal(s2, sums)                    # integers: exact in any order
        else:
            assert max_rel(e2, e) <= bound


def test_the_generator_is_duplicate_free_and_the_last_triple_wins():
    t = tm.hic_like_triples(300)
    i, j, v = tm.upper_cells(t, tm.RESOLUTION, 300)
    assert i.shape[0] == t.shape[0] and (j - i <= 24).sum() > 24 * 200 and (j - i > 24).any()
    twice = numpy.concatenate([t, t[:10] * [1, 1, 0] + [0, 0, 77.0], t[:5, [1, 0, 2]] * [1, 1, 0] + [0, 0, 5.0]])
    i2, j2, v2 = tm.upper_cells(twice, tm.RESOLUTION, 300)
    assert numpy.array_equal(i2, i) and numpy.array_equal(j2, j)
    b = (t[:10, :2] / tm.RESOLUTION).astype(int)
    for r in range(10):
        at = numpy.flatnonzero((i2 == b[r].min()) & (j2 == b[r].max()))[0]
        assert v2[at] == (5.0 if r < 5 else 77.0)
    with pytest.raises(ValueError, match="outside"):
        tm.upper_cells([[301.0 * tm.RESOLUTION, 0.0, 1.0]], tm.RESOLUTION, 300)
    # a pair that touches bin n_bins is legal and dropped
    assert tm.upper_cells([[300.0 * tm.RESOLUTION, 0.0, 1.0]], tm.RESOLUTION, 300)[0].size == 0


# ---- arguments: ValueError on a machine without a GPU, the library never loaded ------------------
T = numpy.array([[0.0, 10000.0, 3.0], [10000.0, 20000.0, 2.0], [0.0, 20000.0, 1.0]])
BAD = [dict(ignore_diags=-1), dict(min_nnz=-1), dict(max_iter=-1), dict(tol=-1e-3),
       dict(tol=float("nan")), dict(tol=float("inf")), dict(row_sum=0.0), dict(row_sum=-1.0),
       dict(row_sum=float("inf"))]


@pytest.fixture
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", refuse)


@pytest.mark.parametrize("kw", BAD, ids=lambda kw: "%s=%r" % next(iter(kw.items())))
def test_bad_arguments_raise_before_the_library_is_loaded(kw, no_library):
    with pytest.raises(ValueError):
        bb.balance_triples(T, 10000, 3, **kw)
    with pytest.raises(ValueError):
        bb.StructureSolver().fit_triples(T, 10000, 3, balance=kw)


def test_bad_triples_and_balance_with_krnorm_raise_before_the_library_is_loaded(no_library):
    for bad in (numpy.zeros((4, 2)), numpy.zeros(6), numpy.zeros((2, 3, 1))):
        with pytest.raises(ValueError, match=r"\(n, 3\)"):
            bb.balance_triples(bad, 10000, 3)
        with pytest.raises(ValueError, match=r"\(n, 3\)"):
            bb.StructureSolver().fit_triples(bad, 10000, 3, balance=True)
    with pytest.raises(ValueError, match="KRnorm"):
        bb.StructureSolver().fit_triples(T, 10000, 3, balance=True, KRnorm=numpy.ones(3))
    with pytest.raises(ValueError, match="KRnorm"):
        bb.StructureSolver().fit_triples(T, 10000, 3, balance=dict(ignore_diags=1),
                                         KRnorm=numpy.ones(3), KRexpected=numpy.ones(3))
    with pytest.raises(ValueError, match="unknown argument"):
        bb.StructureSolver().fit_triples(T, 10000, 3, balance=dict(ignore_diag=1))
    with pytest.raises(ValueError, match="balance must be"):
        bb.StructureSolver().fit_triples(T, 10000, 3, balance="ice")


def test_an_engine_without_a_device_refuses_balance():
    class HostEngine(object):                       # (no set_wish_triples: a CPU test double)
        pass
    with pytest.raises(ValueError, match="engine"):
        bb.StructureSolver(engine=HostEngine).fit_triples(T, 10000, 3, balance=True)


def test_the_names_are_exported():
    assert bb.DeviceTriples is not None and callable(bb.balance_triples)
