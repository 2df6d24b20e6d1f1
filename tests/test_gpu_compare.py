"""GPU: bb_structures_moments / bb_structures_compare / compare_structures (SPEC 2.10) against the
float64 model of tests/_compare_model.py.

The main kernel test uses inputs on which every distance, product and sum is an exact integer
(model.exact_case): the device must then give the model's bits whatever order it sums in, at
every size edge of the pair pass, with every bin used and with a mask that drops the bins at every
tile boundary.  Float structures are held to the model's bounds; every case prints its largest
|err| / bound."""
import functools

import numpy
import pytest

pytestmark = pytest.mark.gpu

T = 256                                                   # kT of bb_compare.hip
EDGES = [2, 3, 5, T - 1, T, T + 1, 2 * T + 1, 3 * T + 1]


def _ptr(a):
    from blueberry_amd import _lib
    return None if a is None else _lib.as_f64_ptr(a)


def _use_ptr(use):
    import ctypes
    return None if use is None else use.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))


def _moments(A, B, use=None):
    """(status, out18) of the C entry; use: uint8 per bin or None."""
    from blueberry_amd import _lib
    out = numpy.zeros(18)
    rc = _lib.load().bb_structures_moments(_ptr(A), _ptr(B), _use_ptr(use), A.shape[0], 0, _ptr(out))
    return rc, out


def _compare(A, B, use, transform, ranks=False, want_ms=False):
    """The C entry's outputs: aligned, bin_dev, profile, bins, rank_sums (None without ranks)."""
    from blueberry_amd import _lib
    n = A.shape[0]
    aligned, dev = numpy.zeros((n, 3)), numpy.zeros(n)
    profile, bins = numpy.full((n, 7), -1.0), numpy.full((n, 2), -1.0)
    rank_sums = numpy.full(4, -1.0) if ranks else None
    ms = numpy.full(5, -1.0) if want_ms else None
    transform = numpy.ascontiguousarray(transform, dtype=numpy.float64)
    _lib.check(_lib.load().bb_structures_compare(_ptr(A), _ptr(B), _use_ptr(use), n, _ptr(transform),
                                                 _lib.BB_CMP_SPEARMAN if ranks else 0, 0, _ptr(aligned),
                                                 _ptr(dev), _ptr(profile), _ptr(bins), _ptr(rank_sums), _ptr(ms)),
               "bb_structures_compare")
    return (aligned, dev, profile, bins, rank_sums) + ((ms,) if want_ms else ())


def _u8(mask):
    return numpy.ascontiguousarray(mask, dtype=numpy.uint8)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _exact(n, masked):
    """(A, B, used, aligned, dev2, profile, bins) of the exact case: made once, never changed."""
    from tests import _compare_model as model
    A, B = model.exact_case(n)
    used = model.edge_mask(n, T) if masked else numpy.ones(n, dtype=bool)
    aligned, dev2 = model.transform(A, B, used, numpy.eye(3), numpy.zeros(3), 1.0)
    return _frozen(A, B, used, aligned, dev2, *model.pair_sums(A, aligned, used))


def _same(got, want, what):
    assert got.shape == want.shape, what
    assert numpy.array_equal(got, want, equal_nan=True), (what, numpy.argwhere(got != want)[:5])


# ---- 1. exact inputs at every size edge ------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("n", EDGES)
def test_exact_inputs_bit_for_bit(n, masked):
    from tests import _compare_model as model
    A, B, used, aligned, dev2, profile, bins = _exact(n, masked)
    got = _compare(A, B, _u8(used) if masked else None, model.IDENTITY13)
    _same(got[0], aligned, "aligned")
    _same(got[1], dev2, "bin_dev")
    _same(got[2], profile, "profile")
    _same(got[3], bins, "bins")
    nu = int(used.sum())
    assert profile[:, 0].sum() == nu * (nu - 1) // 2 and not profile[0].any()
    assert bins[:, 1].sum() == 2 * profile[:, 6].sum()
    if masked and n > T:
        assert not used[[0, T - 1, T, n - 1]].any() and not bins[~used].any()


# ---- 2. float structures -----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _float(n):
    """The float case and its model: A, B, used, moments, their bound, the transform the model's
    moments give, aligned, dev2, profile, bins, profile bound, bins bound."""
    from tests import _compare_model as model
    A, B = model.float_case(n)
    used = model.edge_mask(n, T) if n > 8 else numpy.ones(n, dtype=bool)
    mo, mo_bound = model.moments_and_bounds(A, B, used)
    R, t, s, _ = model.superposition(mo, mirror=True, scale=True)
    tr = numpy.concatenate([R.reshape(9), t, [s]])
    aligned, dev2 = model.transform(A, B, used, R, t, s)
    return _frozen(A, B, used, mo, mo_bound, tr, aligned, dev2, *model.pair_sums_and_bounds(A, aligned, used))


def _within(dev, ref, bound, label):
    err = numpy.abs(dev - ref)
    assert ((bound > 0) | (err == 0)).all(), label
    ratio = err / numpy.where(bound > 0, bound, 1.0)
    print("compare %s: max |err| / bound = %.3g" % (label, float(ratio.max())))
    assert (err <= bound).all(), (label, float(ratio.max()))


@pytest.mark.parametrize("n", [4, 65, T + 1, 2 * T + 1])
def test_float_structures_within_the_bounds(n):
    A, B, used, mo, mo_bound, tr, aligned, dev2, profile, bins, profile_bound, bins_bound = _float(n)
    rc, out = _moments(A, B, _u8(used))
    assert rc == 0 and out[0] == used.sum()
    _within(out, mo, mo_bound, "n=%d moments" % n)
    got = _compare(A, B, _u8(used), tr)
    _same(got[0], aligned, "aligned")                 # the transform's roundings are SPEC's: same bits
    _same(got[1], dev2, "bin_dev")
    for col in range(7):
        _within(got[2][:, col], profile[:, col], profile_bound[:, col], "n=%d profile[%d]" % (n, col))
    for col in range(2):
        _within(got[3][:, col], bins[:, col], bins_bound[:, col], "n=%d bins[%d]" % (n, col))


@pytest.mark.parametrize("mirrored", [False, True])
@pytest.mark.parametrize("n", [4, 65, T + 1, 2 * T + 1])
def test_the_python_call_on_an_exact_similarity_image(n, mirrored):
    import blueberry_amd as bb
    from tests import _compare_model as model
    from tests import _oracle
    A = _oracle.random_walk(n, seed=n)
    B = model.similarity_image(A, seed=n + 5, mirrored=mirrored, scale=0.37)
    rep = bb.compare_structures(A, B, scale=True)
    radius = numpy.sqrt(((A - A.mean(axis=0)) ** 2).sum() / n)
    print("compare image n=%d: rmsd / radius = %.3g, scale err = %.3g"
          % (n, rep.rmsd / radius, abs(rep.scale * 0.37 - 1)))
    assert rep.mirrored == mirrored and rep.n_used == n and rep.n_pairs == n * (n - 1) // 2
    assert abs(rep.scale * 0.37 - 1) <= 1e-12
    assert rep.rmsd <= 1e-12 * radius
    assert numpy.linalg.det(rep.rotation) * (-1 if mirrored else 1) > 0.999999
    assert numpy.abs(rep.aligned - A).max() <= 1e-11 * radius
    assert rep.distance_rmsd <= 1e-11 * radius and rep.distance_pearson > 1 - 1e-12
    assert bb.compare_structures(A, B, mirror=False).mirrored is False
    solver = bb.StructureSolver(n_iter=1)
    solver.structure_ = A
    again = solver.compare(B, scale=True)
    assert numpy.array_equal(again.sums, rep.sums) and again.rmsd == rep.rmsd


# ---- 3. ranks ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _integer(n):
    from tests import _compare_model as model
    A, B = model.integer_case(n)
    used = numpy.ones(n, dtype=bool)
    return _frozen(A, B, used, *model.rank_sums_and_bounds(A, B, used))


@pytest.mark.parametrize("n", [2, 3, 91, 92, 513])
def test_ranks_of_tied_distances(n):
    import blueberry_amd as bb
    from tests import _compare_model as model
    A, B, used, sums, bound = _integer(n)
    got = _compare(A, B, None, model.IDENTITY13, ranks=True)[4]
    m = n * (n - 1) // 2
    assert got[0] == m == sums[0]
    if n in (91, 92):                                 # 91 fills the sort's tile but for one slot, 92 crosses it
        assert (m > model.SORT_TILE) == (n == 92) and m >= model.SORT_TILE - 1
    _within(got[1:], sums[1:], bound[1:], "n=%d rank sums" % n)
    rep = bb.StructureComparison(used, numpy.eye(3), numpy.zeros(3), 1.0, False, B, numpy.zeros(n),
                                 numpy.zeros((n, 7)), numpy.zeros((n, 2)), got)
    if n == 2:                                        # one pair
        assert numpy.isnan(rep.distance_spearman) and numpy.isnan(model.spearman(sums))
        return
    rho, allowed = model.spearman(sums), model.spearman_bound(sums, bound)
    print("compare ranks n=%d: rho = %.15f, |err| = %.3g, bound = %.3g"
          % (n, rep.distance_spearman, abs(rep.distance_spearman - rho), allowed))
    assert abs(rep.distance_spearman - rho) <= allowed
    if n >= 91:                                       # with a mask: the canonical order skips bins
        mask = model.edge_mask(n, 32)
        want, wb = model.rank_sums_and_bounds(A, B, mask)
        got = _compare(A, B, _u8(mask), model.IDENTITY13, ranks=True)[4]
        assert got[0] == want[0]
        _within(got[1:], want[1:], wb[1:], "n=%d masked rank sums" % n)


def test_all_distances_equal_have_no_rank_correlation():
    import blueberry_amd as bb
    from tests import _compare_model as model
    n = 120                                           # 7,140 pairs: one run over two sort tiles
    A, B = model.integer_case(n)
    here = numpy.tile(numpy.array([[3.0, -2.0, 7.0]]), (n, 1))
    got = _compare(here, B, None, model.IDENTITY13, ranks=True)[4]
    assert got[0] == n * (n - 1) // 2 and got[1] == 0.0 and got[3] == 0.0 and got[2] > 0
    rep = bb.compare_structures(here, here + 1.0, spearman=True)
    assert numpy.isnan(rep.distance_spearman) and numpy.isnan(rep.distance_pearson)
    assert rep.rank_sums[0] == rep.n_pairs and rep.rmsd == 0.0


def test_spearman_of_a_chain_against_scipy():
    import scipy.stats
    import blueberry_amd as bb
    from tests import _compare_model as model
    from tests import _oracle
    A = _oracle.random_walk(400, seed=0)
    B = _oracle.noisy_init(A, seed=1, scale=2.0)
    rep = bb.compare_structures(A, B, spearman=True)
    i, j = model.pairs_of(rep.used)
    da, db = model._distance(A, i, j), model._distance(rep.aligned, i, j)
    want = scipy.stats.spearmanr(da, db)[0]
    sums, bound = model.rank_sums_and_bounds(A, rep.aligned, rep.used)
    allowed = model.spearman_bound(sums, bound)
    print("compare chain: rho = %.15f, scipy %.15f, bound %.3g" % (rep.distance_spearman, want, allowed))
    assert rep.rank_sums[0] == 400 * 399 // 2
    assert abs(rep.distance_spearman - want) <= allowed + 4 * model.EPS      # (scipy's own 4 roundings)
    assert 0.5 < want < 0.999999


# ---- 4. the same bits on two calls -------------------------------------------------------------
def test_two_calls_give_the_same_bits():
    A, B, used, mo, _, tr = _float(2 * T + 1)[:6]
    first = (_moments(A, B, _u8(used))[1],) + _compare(A, B, _u8(used), tr, ranks=True)
    second = (_moments(A, B, _u8(used))[1],) + _compare(A, B, _u8(used), tr, ranks=True)
    for a, b in zip(first, second):
        assert numpy.array_equal(a.view(numpy.uint64), b.view(numpy.uint64))
    assert first[5][0] > 0 and first[5][3] != 0


# ---- 5. refusals -------------------------------------------------------------------------------
def test_the_c_entries_refusals_and_n_used():
    from blueberry_amd import _lib
    from tests import _compare_model as model
    lib = _lib.load()
    A, B = model.float_case(40)
    tr = model.IDENTITY13.copy()
    out, dev, profile, bins, ranks = numpy.zeros(18), numpy.zeros(40), numpy.zeros((40, 7)), numpy.zeros((40, 2)), \
        numpy.zeros(4)
    P = _ptr
    for args in ((None, P(B), None, 40, 0, P(out)), (P(A), None, None, 40, 0, P(out)),
                 (P(A), P(B), None, 40, 0, None), (P(A), P(B), None, 1, 0, P(out))):
        assert lib.bb_structures_moments(*args) == _lib.BB_ERR_INVALID
        assert "bb_structures_moments" in _lib.last_error()

    def call(a=A, b=B, n=40, t=tr, flags=0, dev_=dev, profile_=profile, bins_=bins, ranks_=None):
        return lib.bb_structures_compare(P(a), P(b), None, n, P(t), flags, 0, None, P(dev_), P(profile_),
                                         P(bins_), P(ranks_), None)
    for kw in (dict(a=None), dict(b=None), dict(t=None), dict(dev_=None), dict(profile_=None), dict(bins_=None),
               dict(n=1), dict(flags=_lib.BB_CMP_SPEARMAN), dict(flags=2)):
        assert call(**kw) == _lib.BB_ERR_INVALID, kw
        assert "bb_structures_compare" in _lib.last_error()
    assert call(flags=_lib.BB_CMP_SPEARMAN) == _lib.BB_ERR_INVALID and "rank_sums" in _lib.last_error()
    assert call() == _lib.BB_OK and call(flags=_lib.BB_CMP_SPEARMAN, ranks_=ranks) == _lib.BB_OK
    assert ranks[0] == 780
    # 2^32 pairs or more with the flag: refused before anything is allocated
    n_big = 92683
    big = numpy.zeros((n_big, 3))
    assert n_big * (n_big - 1) // 2 >= 2 ** 32
    rc = lib.bb_structures_compare(P(big), P(big), None, n_big, P(tr), _lib.BB_CMP_SPEARMAN, 0, None,
                                   P(numpy.zeros(n_big)), P(numpy.zeros((n_big, 7))), P(numpy.zeros((n_big, 2))),
                                   P(ranks), None)
    assert rc == _lib.BB_ERR_INVALID and "2^32" in _lib.last_error()
    # n_used: the mask and the finite rows
    A2, B2 = A.copy(), B.copy()
    A2[3, 0], B2[4, 2], B2[5, 1] = numpy.nan, numpy.inf, -numpy.inf
    mask = numpy.ones(40, dtype=bool)
    mask[[0, 3, 17]] = False
    rc, got = _moments(A2, B2, _u8(mask))
    used = model.used_bins(A2, B2, mask)
    assert rc == 0 and got[0] == used.sum() == 35
    want, bound = model.moments_and_bounds(A2, B2, used)
    assert (numpy.abs(got - want) <= bound).all()
    rc, got = _moments(A2, B2)
    assert rc == 0 and got[0] == 37
    res = _compare(A2, B2, _u8(mask), tr)
    assert numpy.isnan(res[0][~used]).all() and numpy.isfinite(res[0][used]).all()
    assert res[2][:, 0].sum() == 35 * 34 // 2 and not res[3][~used].any()
