"""No GPU: the numpy model of the q-value rule's sort key (tests/_qvalue_model.py, docs/SPEC.md
2.9.7) against numpy's own stable argsort of float64, `q_values`' argument checks, and the new
names of the C ABI."""
import numpy
import pytest

import blueberry_amd as bb
from blueberry_amd import _lib
from tests import _qvalue_model as qm

LENGTHS = [0, 1, 2, 65, 4097, 262145]


@pytest.mark.parametrize("name", ["bits", "specials", "uniform", "ulp"])
def test_a_stable_sort_by_the_key_is_numpys_stable_argsort(name):
    for m in LENGTHS:
        p = qm.family(name, m)
        assert p.shape == (m,) and p.dtype == numpy.float64
        assert numpy.array_equal(qm.stable_order(p), numpy.argsort(p, kind="stable")), (name, m)


def test_the_families_hold_what_they_are_for():
    bits = qm.family("bits", 4097)
    assert numpy.isnan(bits).any() and (bits < 0).any() and (bits > 0).any()
    k = qm.key(bits)
    for shift in range(0, 64, 8):                                  # every digit of every pass varies
        assert numpy.unique((k >> numpy.uint64(shift)) & numpy.uint64(255)).shape[0] > 200, shift
    sp = qm.family("specials", 4097)
    assert numpy.unique(sp.view(numpy.uint64)).shape[0] == qm.SPECIALS.shape[0]
    ulp = qm.family("ulp", 4097)
    assert numpy.unique(ulp).shape[0] == 256
    assert numpy.unique(qm.key(ulp) >> numpy.uint64(8)).shape[0] == 1    # the lowest digit alone


def test_the_key_of_the_named_values():
    p = numpy.array([numpy.nan, -numpy.nan, 0.0, -0.0, -1.0, 1.0, -numpy.inf, numpy.inf])
    k = qm.key(p)
    b = p.view(numpy.uint64)
    assert k[0] == k[1] == qm.ALL and k[2] == k[3] == qm.TOP
    assert k[4] == ~b[4] and k[5] == (b[5] | qm.TOP)
    assert k[6] < k[4] < k[2] < k[5] < k[7] < k[0]


def test_argument_checks_raise_before_any_device_call(monkeypatch):
    def no_device():
        raise AssertionError("a device call was made")
    monkeypatch.setattr(_lib, "load", no_device)
    with pytest.raises(ValueError, match="real numbers"):
        bb.q_values(["a", "b"])
    with pytest.raises(ValueError, match="real numbers"):
        bb.q_values(numpy.array([1 + 2j]))
    with pytest.raises(ValueError, match="real numbers"):
        bb.q_values(numpy.array([None, 0.5], dtype=object))
    with pytest.raises(ValueError, match="n_tests"):
        bb.q_values([0.1, 0.2], n_tests=-1)
    with pytest.raises(ValueError, match="NaN"):
        bb.FitHiC(resolution=10).fit_transform(bb.ContactMap.from_matrix(numpy.ones((9, 9)), resolution=10),
                                               q_max=numpy.nan)


def test_the_new_names_are_bound():
    for name in ("bb_q_values", "bb_sig_q_values", "bb_sig_read_q", "bb_sig_select"):
        assert name in _lib.SIGNATURES, name
    assert bb.q_values is bb.stats.q_values and "q_values" in bb.__doc__
