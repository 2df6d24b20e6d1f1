"""CPU: the host side of the shortest-path completion (docs/SPEC.md 2.1.1) -- the `complete=`
argument of the fit entry points and the C-ABI surface.  The completion itself runs on the
GPU only (tests/test_gpu_shortest_paths.py)."""
import inspect
import os
import re

import numpy
import pytest

import blueberry_amd as bb
from blueberry_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_complete_argument_is_checked_before_any_device_call():
    m = numpy.ones((4, 4))
    s = bb.StructureSolver()
    for bad in ("bogus", "", 1, True, "shortest_paths"):
        with pytest.raises(ValueError, match="complete"):
            s.fit(m, complete=bad)
        with pytest.raises(ValueError, match="complete"):
            s.fit_many([m, m], complete=bad)
        with pytest.raises(ValueError, match="complete"):
            s.fit_triples(numpy.array([[0.0, 5000.0, 3.0]]), 5000, 4, complete=bad)
    # the option is per fit: the constructor's parameter list is as it was
    assert "complete" not in inspect.signature(bb.StructureSolver.__init__).parameters
    for name in ("fit", "fit_many", "fit_triples"):
        p = inspect.signature(getattr(bb.StructureSolver, name)).parameters
        assert p["complete"].default is None, name


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_complete_none_is_todays_fit_bit_for_bit(dtype):
    from tests import _oracle
    from tests._engines import OracleEngine
    n = 150
    w = _oracle.wish_from_coords(_oracle.random_walk(n))
    hole = numpy.triu(numpy.random.default_rng(5).random((n, n)) < 0.3, 1)
    w[hole | hole.T] = 0.0
    make = lambda: bb.StructureSolver(n_iter=5, dtype=dtype, kind="wish", seed=3, distributed=False,
                                      engine=OracleEngine, degree_steps=True)
    a, b = make().fit(w), make().fit(w, complete=None)
    assert numpy.array_equal(a.structure_, b.structure_) and numpy.array_equal(a.stress_, b.stress_)
    assert not hasattr(b, "completed_unreachable_pairs_")
    many_a, many_b = make().fit_many([w, w[:90, :90]]), make().fit_many([w, w[:90, :90]], complete=None)
    for q in range(2):
        assert numpy.array_equal(many_a.structures_[q], many_b.structures_[q])
        assert numpy.array_equal(many_a.stresses_[q], many_b.stresses_[q])


def test_shortest_paths_is_in_the_header_and_the_binding():
    text = open(os.path.join(ROOT, "include", "blueberry_hip.h")).read()
    decl = re.search(r"BB_API\s+int\s+bb_cm_shortest_paths\s*\(([^)]*)\)", text)
    assert decl, "bb_cm_shortest_paths is not declared in include/blueberry_hip.h"
    args = [a.strip() for a in decl.group(1).split(",")]
    assert len(args) == 5 and args[0].startswith("const bb_cm") and args[1].startswith("bb_cm")
    restype, argtypes = _lib.SIGNATURES["bb_cm_shortest_paths"]
    assert restype is _lib.c_int
    assert argtypes == [_lib.c_void_p, _lib.c_void_p, _lib.c_int, _lib.c_dbl, _lib.p_i64]
    assert getattr(_lib.load(), "bb_cm_shortest_paths") is not None
    assert _lib.load().bb_version() == 100


def test_completion_arguments_are_checked_without_a_device():
    assert bb.shortest_paths is bb.datatypes.shortest_paths
    cm = bb.ContactMap.from_matrix(numpy.ones((3, 3)))
    for call in (lambda **kw: cm.shortest_paths(**kw),
                 lambda **kw: bb.shortest_paths(numpy.ones((3, 3)), **kw)):
        with pytest.raises(ValueError, match="kind"):
            call(kind="p")
        with pytest.raises(ValueError, match="alpha"):
            call(alpha=0.0)
        with pytest.raises(ValueError, match="alpha"):
            call(alpha=-1.0)
    with pytest.raises(ValueError, match="square"):
        bb.shortest_paths(numpy.ones((3, 4)))
    assert cm.matrix.shape == (3, 3) and not cm.is_resident     # nothing was uploaded


def test_sparse_input_is_scattered_as_fit_treats_it():
    """Either triangle names a pair, the last entry of a pair wins, the diagonal is dropped."""
    import scipy.sparse
    from blueberry_amd.datatypes import _dense_from_any
    rows = numpy.array([0, 2, 1, 3, 3, 1])
    cols = numpy.array([1, 0, 0, 3, 2, 0])
    vals = numpy.array([5.0, 7.0, 9.0, 4.0, 2.0, 6.0])
    m = _dense_from_any(scipy.sparse.coo_matrix((vals, (rows, cols)), shape=(4, 4)))
    want = numpy.zeros((4, 4))
    want[0, 1] = want[1, 0] = 6.0       # (0,1) then (1,0) twice: the last one
    want[0, 2] = want[2, 0] = 7.0
    want[2, 3] = want[3, 2] = 2.0
    assert numpy.array_equal(m, want)
