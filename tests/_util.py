"""Test-only: the small helpers that several test files share, one copy of each.  Never imported
by the package."""
import ctypes
import os

import numpy
import pytest


def bits(a):
    """The bit patterns of `a` as float64."""
    return numpy.ascontiguousarray(a, dtype=numpy.float64).view(numpy.uint64)


def same_bits(a, b):
    """Same shape and equal as bit patterns: signed zeros and denormals are told apart, a NaN
    equals itself."""
    return a.shape == b.shape and numpy.array_equal(bits(a), bits(b))


def rel(a, b):
    """max |a - b| relative to the largest |b|."""
    return numpy.abs(a - b).max() / numpy.abs(b).max()


def max_rel(got, want):
    """max |got - want| / |want| over the entries where `want` is a number; the NaN patterns
    must be the same."""
    nan = numpy.isnan(want)
    assert numpy.array_equal(numpy.isnan(got), nan)
    if nan.all():
        return 0.0
    return float(numpy.max(numpy.abs(got[~nan] - want[~nan]) / numpy.abs(want[~nan])))


def host_threads():
    """Threads for a host reference: the CPUs this process may run on, 16 at the most."""
    try:
        return max(1, min(16, len(os.sched_getaffinity(0))))
    except AttributeError:
        return max(1, min(16, os.cpu_count() or 1))


def cu_count():
    """The CU count of device 0 as the library reads it: hipDeviceGetAttribute(
    hipDeviceAttributeMultiprocessorCount = 63) of the HIP runtime the library is bound to."""
    from blueberry_amd import _lib
    _lib.load()
    runtimes = _lib.hip_runtimes_loaded()
    own = [p for p in runtimes if "/torch/" not in p] or runtimes
    hip = ctypes.CDLL(own[0])
    hip.hipDeviceGetAttribute.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_int]
    value = ctypes.c_int(0)
    assert hip.hipDeviceGetAttribute(ctypes.byref(value), 63, 0) == 0 and value.value > 0
    return int(value.value)


@pytest.fixture(params=["row_owner", "units"])
def solver_path(request, monkeypatch):
    """Small one-rank problems (up to 4,096 bins) iterate on the row-owner path (one launch per
    iteration, both triangles resident); BB_ROW_OWNER_MAX=0 sends them down the unit sweep that
    large maps and multi-rank jobs use.  Tests that carry this fixture hold for both."""
    if request.param == "units":
        monkeypatch.setenv("BB_ROW_OWNER_MAX", "0")
    else:
        monkeypatch.delenv("BB_ROW_OWNER_MAX", raising=False)
    return request.param
