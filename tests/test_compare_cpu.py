"""No GPU: what `compare_structures` (docs/SPEC.md 2.10) does on the host -- the names of the C
ABI, the argument checks, the superposition from given moments, and the report derived from given
sums -- and the numpy model of tests/_compare_model.py against scipy and against its own
definitions."""
import os
import re

import numpy
import pytest
import scipy.stats

import blueberry_amd as bb
from blueberry_amd import _lib
from blueberry_amd import compare as cmp
from tests import _compare_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_new_names_are_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "blueberry_hip.h")).read()
    for name in ("bb_structures_moments", "bb_structures_compare"):
        assert name in _lib.SIGNATURES, name
        assert re.search(r"BB_API\s+int\s+%s\s*\(" % name, text), name
    assert re.search(r"BB_CMP_SPEARMAN\s*=\s*%d\b" % _lib.BB_CMP_SPEARMAN, text)
    assert bb.compare_structures is cmp.compare_structures
    assert bb.StructureComparison is cmp.StructureComparison
    assert "compare_structures" in bb.__doc__ and "StructureComparison" in bb.__doc__
    assert callable(bb.StructureSolver.compare)
    assert "bb_compare.hip" in open(os.path.join(ROOT, "build.sh")).read()


def test_argument_checks_raise_before_any_device_call(monkeypatch):
    def no_device():
        raise AssertionError("a device call was made")
    monkeypatch.setattr(_lib, "load", no_device)
    A = numpy.random.default_rng(0).standard_normal((6, 3))
    with pytest.raises(ValueError, match="same n"):
        bb.compare_structures(A, A[:5])
    with pytest.raises(ValueError, match="same n"):
        bb.compare_structures(A[:1], A[:1])
    with pytest.raises(ValueError, match=r"\(n, 3\)"):
        bb.compare_structures(A[:, :2], A[:, :2])
    with pytest.raises(ValueError, match=r"\(n, 3\)"):
        bb.compare_structures(A.reshape(-1), A.reshape(-1))
    with pytest.raises(ValueError, match="real numbers"):
        bb.compare_structures(A.astype(complex), A)
    with pytest.raises(ValueError, match="real numbers"):
        bb.compare_structures(A, A.astype(object))
    with pytest.raises(ValueError, match="mask"):
        bb.compare_structures(A, A, mask=numpy.ones(5, dtype=bool))
    with pytest.raises(ValueError, match="mask"):
        bb.compare_structures(A, A, mask=numpy.ones(6))
    only_one = numpy.zeros(6, dtype=bool)
    only_one[2] = True
    with pytest.raises(ValueError, match="fewer than 2 used"):
        bb.compare_structures(A, A, mask=only_one)
    holes = A.copy()
    holes[1:, 1] = numpy.nan                             # one finite bin left in B
    with pytest.raises(ValueError, match="fewer than 2 used"):
        bb.compare_structures(A, holes)
    many = numpy.zeros((cmp.MAX_SPEARMAN_BINS + 1, 3))
    assert cmp.MAX_SPEARMAN_BINS == 92681
    with pytest.raises(ValueError, match="92681 used bins"):
        bb.compare_structures(many, many, spearman=True)
    with pytest.raises(AssertionError, match="device call"):     # (fine without the ranks)
        bb.compare_structures(many, many)
    with pytest.raises(ValueError, match="none fitted yet"):
        bb.StructureSolver(n_iter=1).compare(A)
    solver = bb.StructureSolver(n_iter=1)
    solver.structure_ = A
    with pytest.raises(ValueError, match="same n"):              # A = structure_
        solver.compare(A[:5])


def test_used_bins_are_the_mask_and_the_finite_rows():
    A = numpy.arange(30.0).reshape(10, 3)
    B = A.copy()
    A[3, 0], B[4, 2], B[5, 1] = numpy.nan, numpy.inf, -numpy.inf
    mask = numpy.ones(10, dtype=bool)
    mask[[0, 3]] = False
    want = numpy.array([0, 1, 1, 0, 0, 0, 1, 1, 1, 1], dtype=bool)
    assert numpy.array_equal(cmp.used_bins(A, B, mask), want)
    assert numpy.array_equal(model.used_bins(A, B, mask), want)
    assert cmp.used_bins(A, B).sum() == 7


# ---- the host step on given moments ---------------------------------------------------------------
CASES = [(False, 1.0, False), (True, 1.0, False), (False, 0.37, True), (True, 0.37, True)]


@pytest.mark.parametrize("mirrored,factor,scale", CASES)
@pytest.mark.parametrize("n", [3, 4, 17, 256, 1025])
def test_superposition_of_an_exact_similarity_image(n, mirrored, factor, scale):
    from tests import _oracle
    A = _oracle.random_walk(n, seed=n)
    B = model.similarity_image(A, seed=n + 1, mirrored=mirrored, scale=factor)
    used = numpy.ones(n, dtype=bool)
    mo, _ = model.moments_and_bounds(A, B, used)
    R, t, s, was_mirrored = cmp.superposition(mo, mirror=True, scale=scale)
    if n == 3:                                   # three bins lie in a plane: its own mirror image
        assert not was_mirrored and numpy.linalg.det(R) > 0.999999
    else:
        assert was_mirrored == mirrored and numpy.linalg.det(R) * (-1 if mirrored else 1) > 0.999999
    assert abs(s * factor - 1) <= 1e-12
    assert numpy.abs(R @ R.T - numpy.eye(3)).max() <= 1e-14
    aligned, dev2 = model.transform(A, B, used, R, t, s)
    radius = numpy.sqrt(mo[7] / n)
    assert numpy.sqrt(dev2.sum() / n) <= 1e-12 * radius
    # the same choice as the model's, which forms both candidates and their residuals
    if n == 3:
        return
    R2, t2, s2, m2 = model.superposition(mo, mirror=True, scale=scale)
    assert m2 == was_mirrored and numpy.abs(R - R2).max() <= 1e-12 and abs(s - s2) <= 1e-12 * s2
    assert numpy.abs(t - t2).max() <= 1e-12 * max(1.0, numpy.abs(t2).max())


def test_mirror_false_refuses_the_mirror_image():
    from tests import _oracle
    A = _oracle.random_walk(200, seed=4)
    B = model.similarity_image(A, seed=8, mirrored=True, scale=1.0)
    used = numpy.ones(200, dtype=bool)
    mo, _ = model.moments_and_bounds(A, B, used)
    R, t, s, was_mirrored = cmp.superposition(mo, mirror=False)
    assert not was_mirrored and numpy.linalg.det(R) > 0.999999 and s == 1.0
    _, dev2 = model.transform(A, B, used, R, t, s)
    radius = numpy.sqrt(mo[7] / 200)
    assert numpy.sqrt(dev2.mean()) > 0.05 * radius               # a rotation cannot undo a mirror
    R, t, s, was_mirrored = cmp.superposition(mo, mirror=True)
    _, dev2 = model.transform(A, B, used, R, t, s)
    assert was_mirrored and numpy.sqrt(dev2.mean()) <= 1e-12 * radius


def test_translation_and_masked_bins():
    from tests import _oracle
    A = _oracle.random_walk(300, seed=2)
    B = A + numpy.array([3.0, -7.0, 11.0])
    used = model.edge_mask(300, tile=64)
    B[~used] += 100.0                                            # the unused bins do not count
    mo, _ = model.moments_and_bounds(A, B, used)
    assert mo[0] == used.sum()
    R, t, s, was_mirrored = cmp.superposition(mo)
    assert not was_mirrored and numpy.abs(R - numpy.eye(3)).max() <= 1e-13
    assert numpy.abs(t + numpy.array([3.0, -7.0, 11.0])).max() <= 1e-12
    aligned, dev2 = model.transform(A, B, used, R, t, s)
    assert numpy.isnan(aligned[~used]).all() and numpy.isnan(dev2[~used]).all()
    assert numpy.isfinite(aligned[used]).all()


# ---- the model ------------------------------------------------------------------------------------
def test_the_models_rho_is_scipys():
    A, B = model.integer_case(64)
    used = numpy.ones(64, dtype=bool)
    i, j = model.pairs_of(used)
    assert i.shape[0] == 2016 and (i < j).all()
    da, db = model._distance(A, i, j), model._distance(B, i, j)
    tied = da.shape[0] - (numpy.unique(da, return_counts=True)[1] == 1).sum()
    assert tied > 1000                                           # ties are the rule here
    sums, bound = model.rank_sums_and_bounds(A, B, used)
    want = scipy.stats.spearmanr(da, db)[0]
    assert abs(model.spearman(sums) - want) <= 4 * model.EPS
    assert sums[0] == 2016 and (bound[1:] > 0).all() and model.spearman_bound(sums, bound) < 1e-11
    r = model.centred_ranks(da)
    assert numpy.array_equal(2 * r, numpy.rint(2 * r)) and r.sum() == 0
    # all distances equal: no variance in the ranking
    same = numpy.zeros((5, 3))
    sums, _ = model.rank_sums_and_bounds(same, A[:5], numpy.ones(5, dtype=bool))
    assert sums[1] == 0 and numpy.isnan(model.spearman(sums))


def test_the_models_pair_sums_are_the_definitions():
    A, B = model.float_case(37)
    used = model.edge_mask(37, tile=16)
    aligned, _ = model.transform(A, B, used, numpy.eye(3), numpy.zeros(3), 1.0)
    profile, bins, pb, bb_ = model.pair_sums_and_bounds(A, aligned, used)
    want_p, want_b = numpy.zeros((37, 7)), numpy.zeros((37, 2))
    for i in range(37):
        for j in range(i + 1, 37):
            if used[i] and used[j]:
                da = numpy.sqrt(((A[i] - A[j]) ** 2).sum())
                db = numpy.sqrt(((B[i] - B[j]) ** 2).sum())
                want_p[j - i] += [1, da, db, da * da, db * db, da * db, (da - db) ** 2]
                want_b[i] += [1, (da - db) ** 2]
                want_b[j] += [1, (da - db) ** 2]
    assert numpy.array_equal(profile[:, 0], want_p[:, 0]) and numpy.array_equal(bins[:, 0], want_b[:, 0])
    assert numpy.allclose(profile, want_p, rtol=1e-12, atol=0) and numpy.allclose(bins, want_b, rtol=1e-12, atol=0)
    assert (pb[profile[:, 0] > 0] > 0).all() and not pb[profile[:, 0] == 0].any()
    assert abs(bins[:, 1].sum() - 2 * profile[:, 6].sum()) <= 1e-12 * bins[:, 1].sum()


def test_the_exact_case_is_exact():
    A, B = model.exact_case(300)
    used = model.edge_mask(300)
    aligned, dev2 = model.transform(A, B, used, numpy.eye(3), numpy.zeros(3), 1.0)
    assert numpy.array_equal(aligned[used], B[used])
    profile, bins = model.pair_sums(A, aligned, used)
    assert numpy.array_equal(profile, numpy.rint(profile)) and profile.max() < 2.0 ** 53
    assert bins[:, 1].sum() == 2 * profile[:, 6].sum()
    assert not used[[0, 255, 256, 299]].any() and not profile[0].any()


@pytest.mark.parametrize("case,masked", [("exact", False), ("float", False), ("exact", True), ("float", True)])
@pytest.mark.parametrize("n", [2, 3, 257, 769])
def test_the_sum_by_diagonals_is_pair_sums_bit_for_bit(n, case, masked):
    A, B = model.exact_case(n) if case == "exact" else model.float_case(n)
    used = model.edge_mask(n) if masked else numpy.ones(n, dtype=bool)
    if case == "exact":
        aligned, _ = model.transform(A, B, used, numpy.eye(3), numpy.zeros(3), 1.0)
    else:
        aligned, _ = model.transform(A, B, used, model.rotation(3), numpy.array([1.0, -2.0, 0.5]), 2.7)
    want = model.pair_sums(A, aligned, used, with_magnitudes=True)
    got = model.pair_sums_by_diagonal(A, aligned, used, with_magnitudes=True)
    assert len(got) == 4
    for g, w, what in zip(got, want, ("profile", "bins", "profile magnitudes", "bin magnitudes")):
        assert g.shape == w.shape and g.dtype == w.dtype == numpy.float64, what
        assert numpy.array_equal(g, w), (what, numpy.argwhere(g != w)[:5])
    for g, w in zip(model.pair_sums_by_diagonal(A, aligned, used), want[:2]):
        assert numpy.array_equal(g, w)
    for g, w in zip(model.pair_sums_and_bounds_by_diagonal(A, aligned, used),
                    model.pair_sums_and_bounds(A, aligned, used)):
        assert numpy.array_equal(g, w)
    nu = int(used.sum())
    assert got[0][:, 0].sum() == nu * (nu - 1) // 2 and got[1][:, 0].sum() == nu * (nu - 1)
    if masked and n > 3:
        assert nu < n - 2 and not got[1][~used].any()


@pytest.mark.parametrize("n,masked", [(2, False), (1025, False), (1025, True), (2049, True), (263169, True)])
def test_the_exact_moments_case_is_exact(n, masked):
    used = model.block_mask(n) if masked else numpy.ones(n, dtype=bool)
    A, B = model.exact_moments_case(n, used)
    idx = numpy.nonzero(used)[0]
    nu = idx.shape[0]
    assert numpy.array_equal(A, numpy.rint(A)) and numpy.array_equal(B, numpy.rint(B))
    assert A.min() >= 0 and B.min() >= 0 and max(A.max(), B.max()) < 1000 + nu
    assert max(numpy.delete(A, idx[-1], axis=0).max(), numpy.delete(B, idx[-1], axis=0).max()) < 1000
    out, _ = model.moments_and_bounds(A, B, used)
    assert numpy.array_equal(out, numpy.rint(out)) and numpy.abs(out).max() < 2.0 ** 53
    # the same 18 numbers in integers
    a, b = A[used].astype(numpy.int64), B[used].astype(numpy.int64)
    assert not (a.sum(axis=0) % nu).any() and not (b.sum(axis=0) % nu).any()
    da, db = a - a.sum(axis=0) // nu, b - b.sum(axis=0) // nu
    want = numpy.concatenate([[nu], a.sum(axis=0) // nu, b.sum(axis=0) // nu, [(da * da).sum(), (db * db).sum()],
                              (db.T @ da).reshape(9)])
    assert numpy.array_equal(out, want.astype(numpy.float64))
    assert n == 2 or (out[7] > 0 and out[8] > 0 and numpy.abs(out[9:]).min() > 0)
    if masked and n > 2048:                          # more than the edges: whole blocks are out
        assert nu < n - 1280


def test_the_block_mask_drops_whole_blocks():
    for n in (700, 1000, 2049, 4097):
        mask, edges = model.block_mask(n), model.edge_mask(n)
        assert not mask[768:2048].any() and not (mask & ~edges).any()
        keep = numpy.ones(n, dtype=bool)
        keep[768:2048] = False
        assert numpy.array_equal(mask[keep], edges[keep])
    assert model.block_mask(4097)[[767, 2048]].tolist() == [False, False]        # (tile edges)
    assert model.block_mask(4097)[2049:2304].sum() > 200
    assert numpy.array_equal(model.block_mask(3000, blocks=((10, 20),))[5:25],
                             model.edge_mask(3000)[5:25] & ~((numpy.arange(5, 25) >= 10) & (numpy.arange(5, 25) < 20)))


# ---- the report -----------------------------------------------------------------------------------
def test_the_report_derived_from_given_sums():
    n = 50
    A, B = model.float_case(n)
    used = model.edge_mask(n, tile=16)
    mo, _ = model.moments_and_bounds(A, B, used)
    R, t, s, mirrored = cmp.superposition(mo, scale=True)
    aligned, dev2 = model.transform(A, B, used, R, t, s)
    profile, bins = model.pair_sums(A, aligned, used)
    ranks, _ = model.rank_sums_and_bounds(A, aligned, used)
    rep = bb.StructureComparison(used, R, t, s, mirrored, aligned, dev2, profile, bins, ranks)
    i, j = model.pairs_of(used)
    da, db = model._distance(A, i, j), model._distance(aligned, i, j)
    assert rep.n_used == used.sum() and rep.n_pairs == da.shape[0] and rep.mirrored
    assert abs(rep.scale * 0.37 - 1) < 0.05
    assert abs(rep.rmsd - numpy.sqrt(((A - aligned)[used] ** 2).sum() / used.sum())) <= 1e-14 * rep.rmsd
    assert numpy.isnan(rep.deviation[~used]).all()
    assert numpy.allclose(rep.deviation[used], numpy.sqrt(((A - aligned)[used] ** 2).sum(axis=1)), rtol=1e-14)
    assert abs(rep.distance_rmsd - numpy.sqrt(((da - db) ** 2).mean())) <= 1e-13 * rep.distance_rmsd
    assert abs(rep.distance_pearson - numpy.corrcoef(da, db)[0, 1]) <= 1e-12
    assert abs(rep.distance_spearman - scipy.stats.spearmanr(da, db)[0]) <= 1e-14
    k = 3
    at_k = (j - i) == k
    assert rep.pairs[k] == at_k.sum() and rep.pairs[0] == 0 and numpy.isnan(rep.mean_distance_a[0])
    assert abs(rep.mean_distance_a[k] - da[at_k].mean()) <= 1e-13 * da[at_k].mean()
    assert abs(rep.mean_distance_b[k] - db[at_k].mean()) <= 1e-13 * db[at_k].mean()
    assert abs(rep.rms_difference[k] - numpy.sqrt(((da - db)[at_k] ** 2).mean())) <= 1e-12 * rep.rms_difference[k]
    assert rep.bin_pairs.sum() == 2 * rep.n_pairs and (rep.bin_pairs[~used] == 0).all()
    assert abs(rep.bin_distance_error.sum() - 2 * profile[:, 6].sum()) <= 1e-12 * profile[:, 6].sum()
    # without ranks, and with rankings that have no variance
    assert numpy.isnan(bb.StructureComparison(used, R, t, s, mirrored, aligned, dev2, profile, bins).distance_spearman)
    flat = bb.StructureComparison(used, R, t, s, mirrored, aligned, dev2, profile, bins, [da.shape[0], 0.0, 5.0, 0.0])
    assert numpy.isnan(flat.distance_spearman)
    one = bb.StructureComparison(used, R, t, s, mirrored, aligned, dev2, profile, bins, [1.0, 0.0, 0.0, 0.0])
    assert numpy.isnan(one.distance_spearman)
    with pytest.raises(ValueError, match=r"\(n, 7\)"):
        bb.StructureComparison(used, R, t, s, mirrored, aligned, dev2, profile[:, :6], bins)
