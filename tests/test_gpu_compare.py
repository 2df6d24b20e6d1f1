"""GPU: bb_structures_moments / bb_structures_compare / compare_structures (SPEC 2.10) against the
float64 model of tests/_compare_model.py.

The main kernel test uses inputs on which every distance, product and sum is an exact integer
(model.exact_case): the device must then give the model's bits whatever order it sums in, at
every size edge of the pair pass, with every bin used and with a mask that drops the bins at every
tile boundary.  Float structures are held to the model's bounds; every case prints its largest
|err| / bound.

The sections from 6 on run the same checks where the kernels change shape with size, around these
constants of bb_compare.hip; every test recomputes the launch geometry it is there for from n by
the host code's formulas and asserts it, so it says which regime it is in:
  kChunkSplit 16      a chunk of cmp_pairs_kernel holds ceil(nb / 16) tiles, nb = ceil(n / kT): one
                      up to n = 4,096, two from 4,097, three from 8,193 (the loop over a chunk's
                      tiles, the barrier between their LDS strips, two diagonals summed across tiles)
  kMomentBins 1,024   bins per workgroup of cmp_sum_kernel / cmp_centred_kernel: a second workgroup,
                      and a second partial for cmp_reduce_kernel, from n = 1,025
  the 256-stride      of cmp_reduce_kernel over the partials (g += 256): a second turn from 257
                      workgroups, n = 262,145
  kRankBlocks 2,048   most workgroups of cmp_rank_sum_kernel: from 1,025 used bins (524,800 pairs) a
                      thread adds more than one place (p += 256), workgroups past the last place
                      are empty, and cmp_reduce_kernel<3> adds 2,048 partials
and with model.block_mask, which leaves a tile, a chunk and a moment workgroup without a used bin.
The pair sums of these sizes come from model.pair_sums_by_diagonal (pair_sums' bits without the
list of all pairs), the moments from model.exact_moments_case, on which all 18 are integers."""
import functools

import numpy
import pytest

pytestmark = pytest.mark.gpu

T = 256                                                   # kT of bb_compare.hip
EDGES = [2, 3, 5, T - 1, T, T + 1, 2 * T + 1, 3 * T + 1]
CHUNK_SPLIT, MOMENT_BINS, RANK_BLOCKS, REDUCE_STRIDE = 16, 1024, 2048, 256     # kChunkSplit, kMomentBins, ...


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


# ---- 6. the pair pass with several tiles in a chunk ---------------------------------------------
def _chunks(n):
    """(per_chunk, [(D, I_begin, I_end)]) of bb_structures_compare's host code."""
    nb = -(-n // T)
    per = -(-nb // CHUNK_SPLIT)
    return per, [(D, I, min(I + per, nb - D)) for D in range(nb) for I in range(0, nb - D, per)]


def _mask_of(n, kind):
    from tests import _compare_model as model
    return {"none": lambda: numpy.ones(n, dtype=bool), "edge": lambda: model.edge_mask(n, T),
            "block": lambda: model.block_mask(n, T)}[kind]()


@functools.lru_cache(maxsize=None)
def _exact_by_diagonal(n, kind):
    """_exact at the sizes pair_sums does not reach: (A, B, used, aligned, dev2, profile, bins)."""
    from tests import _compare_model as model
    A, B = model.exact_case(n)
    used = _mask_of(n, kind)
    aligned, dev2 = model.transform(A, B, used, numpy.eye(3), numpy.zeros(3), 1.0)
    return _frozen(A, B, used, aligned, dev2, *model.pair_sums_by_diagonal(A, aligned, used))


#            n: per_chunk, chunks, chunks of one tile
GEOMETRY = {4096: (1, 136, 136), 4097: (2, 81, 9), 8193: (3, 198, 11)}


@pytest.mark.parametrize("kind", ["none", "edge", "block"])
@pytest.mark.parametrize("n", sorted(GEOMETRY))
def test_exact_inputs_bit_for_bit_with_several_tiles_in_a_chunk(n, kind):
    from tests import _compare_model as model
    per, chunks = _chunks(n)
    tiles = [end - begin for _, begin, end in chunks]
    assert (per, len(chunks), tiles.count(1)) == GEOMETRY[n] and max(tiles) == per
    assert n == 4096 or (per > 1 and 1 in tiles and tiles.count(per) > 1)    # one-tile chunks beside longer ones
    A, B, used, aligned, dev2, profile, bins = _exact_by_diagonal(n, kind)
    got = _compare(A, B, None if kind == "none" else _u8(used), model.IDENTITY13)
    _same(got[0], aligned, "aligned")
    _same(got[1], dev2, "bin_dev")
    _same(got[2], profile, "profile")
    _same(got[3], bins, "bins")
    nu = int(used.sum())
    assert profile[:, 0].sum() == nu * (nu - 1) // 2 and not profile[0].any()
    assert bins[:, 1].sum() == 2 * profile[:, 6].sum()
    assert profile[n - 1, 0] == (kind == "none") and profile.max() < 2.0 ** 53
    if kind != "none":
        assert not used[[0, T - 1, T, n - 1]].any() and not bins[~used].any() and not got[3][~used].any()
    if kind == "block":                               # a tile, a chunk and more without a used bin
        assert not used[768:2048].any() and not got[3][768:2048].any() and nu < n - 1280
        empty = [c for c in chunks if c[0] == 0 and not used[c[1] * T:c[2] * T].any()]
        assert empty and max(end - begin for _, begin, end in empty) == per


@functools.lru_cache(maxsize=None)
def _float_by_diagonal(n):
    """_float through the diagonal route (the same tuple)."""
    from tests import _compare_model as model
    A, B = model.float_case(n)
    used = model.edge_mask(n, T)
    mo, mo_bound = model.moments_and_bounds(A, B, used)
    R, t, s, _ = model.superposition(mo, mirror=True, scale=True)
    tr = numpy.concatenate([R.reshape(9), t, [s]])
    aligned, dev2 = model.transform(A, B, used, R, t, s)
    return _frozen(A, B, used, mo, mo_bound, tr, aligned, dev2,
                   *model.pair_sums_and_bounds_by_diagonal(A, aligned, used))


def test_float_structures_within_the_bounds_with_two_tiles_in_a_chunk():
    n = 16 * T + 1
    assert _chunks(n)[0] == 2
    A, B, used, mo, mo_bound, tr, aligned, dev2, profile, bins, profile_bound, bins_bound = _float_by_diagonal(n)
    got = _compare(A, B, _u8(used), tr)
    _same(got[0], aligned, "aligned")
    _same(got[1], dev2, "bin_dev")
    for col in range(7):
        _within(got[2][:, col], profile[:, col], profile_bound[:, col], "n=%d profile[%d]" % (n, col))
    for col in range(2):
        _within(got[3][:, col], bins[:, col], bins_bound[:, col], "n=%d bins[%d]" % (n, col))
    assert (profile_bound[1:n - 2 * T, 1:] > 0).all() and profile[:, 0].sum() == used.sum() * (used.sum() - 1) // 2


# ---- 7. the moments with several workgroups ------------------------------------------------------
MOMENT_EDGES = [MOMENT_BINS - 1, MOMENT_BINS, MOMENT_BINS + 1, 2 * MOMENT_BINS + 1,
                REDUCE_STRIDE * MOMENT_BINS, REDUCE_STRIDE * MOMENT_BINS + 1]


def _moment_geometry(n):
    """(workgroups of the moment kernels, turns of cmp_reduce_kernel's loop over their partials)."""
    groups = -(-n // MOMENT_BINS)
    return groups, -(-groups // REDUCE_STRIDE)


@functools.lru_cache(maxsize=None)
def _exact_moments(n, kind):
    from tests import _compare_model as model
    used = _mask_of(n, kind)
    A, B = model.exact_moments_case(n, used)
    return _frozen(A, B, used, model.moments_and_bounds(A, B, used)[0])


@pytest.mark.parametrize("n,kind", [(n, "none") for n in MOMENT_EDGES]
                         + [(n, "block") for n in MOMENT_EDGES if n > 2047])
def test_exact_moments_bit_for_bit(n, kind):
    assert _moment_geometry(n) == {1023: (1, 1), 1024: (1, 1), 1025: (2, 1), 2049: (3, 1), 262144: (256, 1),
                                   262145: (257, 2)}[n]
    A, B, used, want = _exact_moments(n, kind)
    assert numpy.array_equal(want, numpy.rint(want)) and numpy.abs(want).max() < 2.0 ** 53 and want[0] == used.sum()
    assert want[7] > 0 and want[8] > 0 and want[9:].all()
    if kind == "block":                               # the second workgroup has no used bin
        assert not used[MOMENT_BINS:2 * MOMENT_BINS].any() and used[:MOMENT_BINS].any()
        assert n == 2 * MOMENT_BINS + 1 or used[2 * MOMENT_BINS:].any()     # (2,049: the third has none either)
    rc, got = _moments(A, B, None if kind == "none" else _u8(used))
    assert rc == 0
    _same(got, want, "moments")


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("n", [MOMENT_BINS + 1, REDUCE_STRIDE * MOMENT_BINS + 1])
def test_float_moments_within_the_bounds(n, masked):
    from tests import _compare_model as model
    assert _moment_geometry(n) == {1025: (2, 1), 262145: (257, 2)}[n]
    A, B = model.float_case(n)
    used = _mask_of(n, "edge" if masked else "none")
    # 1,025 bins: the second workgroup's one bin is used, or, under the mask, it has none
    assert used[MOMENT_BINS:].sum() == (0 if masked else 1) or n > MOMENT_BINS + 1
    want, bound = model.moments_and_bounds(A, B, used)
    rc, got = _moments(A, B, _u8(used) if masked else None)
    assert rc == 0 and got[0] == want[0] == used.sum()
    _within(got, want, bound, "n=%d%s moments" % (n, " masked" if masked else ""))


# ---- 8. the ranks with several places per thread -----------------------------------------------
def _rank_geometry(m):
    """(workgroups, places per workgroup, workgroups without a place) of cmp_rank_sum_kernel."""
    def ceil_div(a, b):
        return -(-a // b)
    groups = min(ceil_div(m, 256), RANK_BLOCKS)
    per = 256 * ceil_div(ceil_div(m, groups), 256)
    return groups, per, groups - ceil_div(m, per)


@functools.lru_cache(maxsize=None)
def _thinned(n, n_used):
    """integer_case(n) and a mask that keeps n_used bins: edge_mask less a seeded choice."""
    from tests import _compare_model as model
    A, B = model.integer_case(n)
    used = model.edge_mask(n, T)
    idx = numpy.nonzero(used)[0]
    used[numpy.random.default_rng(n).choice(idx, idx.shape[0] - n_used, replace=False)] = False
    return _frozen(A, B, used, *model.rank_sums_and_bounds(A, B, used))


def _check_ranks(A, B, used, sums, bound, got, label):
    import blueberry_amd as bb
    from tests import _compare_model as model
    n, m = A.shape[0], int(used.sum()) * (int(used.sum()) - 1) // 2
    assert got[0] == m == sums[0]
    assert sums[1] > 2.0 ** 53 and sums[2] > 2.0 ** 53        # (no bits to ask for)
    _within(got[1:], sums[1:], bound[1:], "%s rank sums" % label)
    rep = bb.StructureComparison(used, numpy.eye(3), numpy.zeros(3), 1.0, False, B, numpy.zeros(n),
                                 numpy.zeros((n, 7)), numpy.zeros((n, 2)), got)
    rho, allowed = model.spearman(sums), model.spearman_bound(sums, bound)
    print("compare ranks %s: rho = %.15f, |err| = %.3g, bound = %.3g"
          % (label, rep.distance_spearman, abs(rep.distance_spearman - rho), allowed))
    assert abs(rep.distance_spearman - rho) <= allowed and 0.5 < rho < 1


#                 used bins: workgroups, places per workgroup, empty workgroups
RANK_GEOMETRY = {1024: (2046, 256, 0), 1025: (2048, 512, 1023), 1448: (2048, 512, 1), 1449: (2048, 768, 682)}


@pytest.mark.parametrize("n", sorted(RANK_GEOMETRY))
def test_ranks_with_several_places_per_thread(n):
    from tests import _compare_model as model
    assert _rank_geometry(n * (n - 1) // 2) == RANK_GEOMETRY[n]
    A, B, used, sums, bound = _integer(n)
    got = _compare(A, B, None, model.IDENTITY13, ranks=True)[4]
    _check_ranks(A, B, used, sums, bound, got, "n=%d" % n)


def test_ranks_of_1025_used_bins_under_a_mask():
    from tests import _compare_model as model
    n, n_used = 1300, 1025
    A, B, used, sums, bound = _thinned(n, n_used)
    assert used.sum() == n_used and not used[[0, T - 1, T, n - 1]].any()
    assert _rank_geometry(n_used * (n_used - 1) // 2) == RANK_GEOMETRY[n_used]
    got = _compare(A, B, _u8(used), model.IDENTITY13, ranks=True)[4]
    _check_ranks(A, B, used, sums, bound, got, "n=%d, %d used" % (n, n_used))


def test_all_distances_equal_over_129_sort_tiles():
    from tests import _compare_model as model
    n = 1025                                          # 524,800 pairs: one run of ties
    m = n * (n - 1) // 2
    assert -(-m // model.SORT_TILE) == 129 and _rank_geometry(m) == RANK_GEOMETRY[n]
    B = _integer(n)[1]
    here = numpy.tile(numpy.array([[3.0, -2.0, 7.0]]), (n, 1))
    got = _compare(here, B, None, model.IDENTITY13, ranks=True)[4]
    assert got[0] == m and got[1] == 0.0 and got[3] == 0.0 and got[2] > 0


# ---- 9. the Python call at these sizes ---------------------------------------------------------
@pytest.mark.parametrize("mirrored", [False, True])
def test_the_python_call_on_a_masked_similarity_image_of_4097_bins(mirrored):
    import blueberry_amd as bb
    from tests import _compare_model as model
    from tests import _oracle
    n = 16 * T + 1
    A = _oracle.random_walk(n, seed=n)
    B = model.similarity_image(A, seed=n + 5, mirrored=mirrored, scale=0.37)
    mask = model.block_mask(n, T)
    nu = int(mask.sum())
    rep = bb.compare_structures(A, B, mask=mask, scale=True)
    radius = numpy.sqrt(((A[mask] - A[mask].mean(axis=0)) ** 2).sum() / nu)
    print("compare image n=%d: rmsd / radius = %.3g, scale err = %.3g"
          % (n, rep.rmsd / radius, abs(rep.scale * 0.37 - 1)))
    assert numpy.array_equal(rep.used, mask) and nu < n - 1280
    assert rep.mirrored == mirrored and rep.n_used == nu and rep.n_pairs == nu * (nu - 1) // 2
    assert abs(rep.scale * 0.37 - 1) <= 1e-12
    assert rep.rmsd <= 1e-12 * radius
    assert numpy.linalg.det(rep.rotation) * (-1 if mirrored else 1) > 0.999999
    assert numpy.isnan(rep.aligned[~mask]).all() and numpy.abs(rep.aligned - A)[mask].max() <= 1e-11 * radius
    assert rep.distance_rmsd <= 1e-11 * radius and rep.distance_pearson > 1 - 1e-12
    assert rep.bin_pairs[mask].min() == nu - 1 == rep.bin_pairs.max() and not rep.bin_pairs[~mask].any()
    assert bb.compare_structures(A, B, mask=mask, mirror=False).mirrored is False
    solver = bb.StructureSolver(n_iter=1)
    solver.structure_ = A
    again = solver.compare(B, mask=mask, scale=True)
    assert numpy.array_equal(again.sums, rep.sums) and again.rmsd == rep.rmsd


def test_the_python_calls_spearman_at_1449_bins():
    import blueberry_amd as bb
    from tests import _compare_model as model
    n = 1449
    A, B = _integer(n)[:2]
    rep = bb.compare_structures(A, B, spearman=True)
    m = n * (n - 1) // 2
    assert rep.n_used == n and rep.rank_sums[0] == m == rep.n_pairs and _rank_geometry(m) == RANK_GEOMETRY[n]
    sums, bound = model.rank_sums_and_bounds(A, rep.aligned, rep.used)
    _within(rep.rank_sums[1:], sums[1:], bound[1:], "n=%d rank sums of the call" % n)
    rho, allowed = model.spearman(sums), model.spearman_bound(sums, bound)
    print("compare call n=%d: rho = %.15f, model %.15f, bound %.3g" % (n, rep.distance_spearman, rho, allowed))
    assert abs(rep.distance_spearman - rho) <= allowed and 0.5 < rho < 1


# ---- 10. the same bits on two calls at these sizes ---------------------------------------------
def _bits(arrays):
    return [a.view(numpy.uint64) for a in arrays]


def test_two_calls_give_the_same_bits_with_two_tiles_in_a_chunk():
    n = 16 * T + 1
    A, B, used, mo, _, tr = _float_by_diagonal(n)[:6]
    first = (_moments(A, B, _u8(used))[1],) + _compare(A, B, _u8(used), tr)[:4]
    second = (_moments(A, B, _u8(used))[1],) + _compare(A, B, _u8(used), tr)[:4]
    for a, b in zip(_bits(first), _bits(second)):
        assert numpy.array_equal(a, b)
    assert first[0][0] == used.sum() and first[3][:, 0].sum() == used.sum() * (used.sum() - 1) // 2


def test_two_calls_give_the_same_bits_with_three_places_per_thread():
    from tests import _compare_model as model
    n = 1449
    assert _rank_geometry(n * (n - 1) // 2)[1] == 3 * 256
    A, B = _integer(n)[:2]
    first = _compare(A, B, None, model.IDENTITY13, ranks=True)
    second = _compare(A, B, None, model.IDENTITY13, ranks=True)
    for a, b in zip(_bits(first), _bits(second)):
        assert numpy.array_equal(a, b)
    assert first[4][0] == n * (n - 1) // 2 and first[4][3] != 0
