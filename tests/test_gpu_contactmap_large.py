"""GPU: the ContactMap-side routines ABOVE the sizes at which they change code path -- the
sizes the small-map tests of tests/test_gpu_parity.py stop short of.

  symv          `symv_upper_kernel` / `symv_reduce_kernel` cut the upper triangle into column
                segments of 4,096: from d = 4,097 on there is more than one segment, the work
                list has two indices, the column range of an item is clamped on both sides and
                the reduce walks "segments s0.., then row blocks".  Checked EXACTLY: integer
                inputs whose every partial sum is an integer below 2^44 (any order of addition
                gives the same float64), and unit vectors (one product by 1.0 plus zeros).
  eigenvector   from d = 4,096 on the Gram-Schmidt dots and beta are formed in 16 segments per
                vector (`basis_dots_kernel` with gridDim.y = 16, summed by
                `lanczos_scalars_kernel`).  Against scipy.sparse.linalg.eigsh(m, k=1), the
                reference project's own call, with the tolerances of the small-map test, and
                against the residual of the returned pair in numpy.longdouble.
  correlation   every instantiation of `center_rows_reg_kernel<CH>`, CH = 4, 8, 16, 24, 32
                (2,048 <= d <= 32,768), and both sides of the switch from `center_rows_kernel`.
                Against numpy.corrcoef; at the two largest sizes against the same formula on a
                sample of rows (tests/_large_maps.py, checked against corrcoef on the CPU).
  scratch       small calls after a large one on the grow-only per-device scratch give the bits
                of the same calls on a fresh scratch.

The inputs, the host references and the properties of both that the tolerances rest on are in
tests/_large_maps.py and tests/test_contactmap_large_inputs_cpu.py.

NOT covered: the two-pass fallback of `bb_cm_correlation` above d = 32,768 (`center_rows_kernel`
again).  It needs a 26 GB working set and a reference nobody can compute in seconds.

Every toleranced figure is printed before it is asserted (`pytest -s`)."""
import time

import numpy
import pytest

import blueberry_amd as bb
from blueberry_amd import _lib
from tests import _large_maps as lm
from tests._util import bits

pytestmark = pytest.mark.gpu

TOL = 1e-13           # ContactMap.eigenvector's default


def symv(dev, x):
    """bb_cm_symv on a resident handle."""
    x = numpy.ascontiguousarray(x, dtype=numpy.float64)
    assert x.shape == (dev.d,)
    y = numpy.full(dev.d, numpy.nan)
    _lib.check(dev._lib.bb_cm_symv(dev._h, _lib.as_f64_ptr(x), _lib.as_f64_ptr(y)), "bb_cm_symv")
    return y


SYMV_SIZES = [4095, 4096,      # the last one-segment sizes
              4097,            # a second segment one column wide
              4161,            # row block 65 lies wholly inside segment 1
              8192,            # two full segments
              8193]            # the third segment begins


# ---- 1. symv: exact ----------------------------------------------------------------------------
@pytest.mark.parametrize("d", SYMV_SIZES)
def test_symv_integer_inputs_exact(d):
    """Entries in [1, 2^20), x in [-1024, 1024], all integers: y must EQUAL M @ x.  A misrouted,
    doubled or dropped element changes an integer."""
    rng = numpy.random.default_rng(d)
    m = lm.integer_symmetric(d, rng)
    dev = bb.ContactMap.from_matrix(m)._resident()
    for _ in range(2):
        x = lm.integer_vector(d, rng)
        y, want = symv(dev, x), m @ x
        wrong = numpy.flatnonzero(y != want)
        assert wrong.size == 0, (d, wrong[:8], y[wrong[:8]], want[wrong[:8]])
        assert numpy.array_equal(y, want)


@pytest.mark.parametrize("d", SYMV_SIZES)
def test_symv_unit_vectors_give_the_columns_bit_for_bit(d):
    """symv(e_j) on the real-valued Hi-C-like map is column j: one product by 1.0 plus zeros."""
    m = lm.hic_matrix(d)
    dev = bb.ContactMap.from_matrix(m)._resident()
    for j in (0, 63, 64, 4095, 4096, d - 1):
        if j >= d:
            continue
        e = numpy.zeros(d)
        e[j] = 1.0
        y = symv(dev, e)
        wrong = numpy.flatnonzero(bits(y) != bits(m[:, j]))
        assert wrong.size == 0, (d, j, wrong[:8], y[wrong[:8]], m[wrong[:8], j])


def test_symv_across_filter_on_one_handle():
    """The number of column segments goes 3 -> 2 -> 1 on ONE handle, whose work list and
    partial-sum buffer are rebuilt in the same grow-only allocation: 8,193 bins, `filter(0)` to
    4,097, more bins zeroed by uploading into the same handle, `filter(0)` to 4,000.  Exact
    against numpy on the host matrix at every stage.

    This is also the one place where a partial sum read from a slot that nobody wrote shows: a
    fresh allocation is all zeros, so on a fresh handle such a read adds 0.  Here the work list
    in front of the partial sums shrinks from 321 items to 129, the sums move up by 192 doubles,
    and the slots of rows 4,096.. in segment 0 -- which no work item writes -- hold row sums of
    the 8,193-bin map."""
    rng = numpy.random.default_rng(81930)
    d0 = 8193
    dead_a = numpy.sort(rng.choice(d0, size=d0 - 4097, replace=False))
    m0 = lm.integer_symmetric(d0, rng, dead_a)
    cm = bb.ContactMap.from_matrix(m0)
    dev = cm._resident()

    def check(m):
        assert dev.d == m.shape[0] and cm._resident() is dev
        x = lm.integer_vector(m.shape[0], rng)
        y, want = symv(dev, x), m @ x
        wrong = numpy.flatnonzero(y != want)
        assert wrong.size == 0, (m.shape[0], wrong[:8], y[wrong[:8]], want[wrong[:8]])

    check(m0)                                                       # 3 segments
    cm.filter(0)
    live_a = numpy.setdiff1d(numpy.arange(d0), dead_a)
    m1 = numpy.ascontiguousarray(m0[numpy.ix_(live_a, live_a)])
    assert cm.shape == (4097, 4097) and numpy.array_equal(cm.to_host(), m1)
    check(m1)                                                       # 2 segments
    dead_b = numpy.sort(rng.choice(4097, size=97, replace=False))
    m2 = m1.copy()
    m2[dead_b, :] = 0.0
    m2[:, dead_b] = 0.0
    _lib.check(dev._lib.bb_cm_upload(dev._h, _lib.as_f64_ptr(m2), 4097), "bb_cm_upload")
    check(m2)                                                       # same edge, same work list
    cm.filter(0)
    live_b = numpy.setdiff1d(numpy.arange(4097), dead_b)
    m3 = numpy.ascontiguousarray(m2[numpy.ix_(live_b, live_b)])
    assert cm.shape == (4000, 4000) and numpy.array_equal(cm.to_host(), m3)
    check(m3)                                                       # 1 segment


# ---- 2. eigenvector at the two-stage switch ----------------------------------------------------
def check_eigenpair(cm, v, m, label):
    """The assertions of test_contactmap_eigenvector_vs_scipy, with eigsh as the reference, plus
    the long-double residual of the returned pair: the routine stops at its own estimate
    <= tol |theta|; the factor 10 is for the rounding of the Lanczos relation, about
    eps * norm(M) * 48 = 1e-14 |theta| here."""
    theta = cm.eigenvalue_
    w, U = lm.eigsh_largest(m, k=1)
    u = lm.fix_sign(U[:, 0])
    res, _ = lm.residual_longdouble(m, theta, v)
    print("%s: eigenvalue rel err %.2e, vector err %.2e, |norm - 1| %.1e, long-double residual "
          "%.2e |theta| (reported %.2e), %d products"
          % (label, abs(theta / w[0] - 1), numpy.abs(v - u).max(), abs(numpy.linalg.norm(v) - 1),
             res / abs(theta), cm.eigen_residual_ / abs(theta), cm.eigen_matvecs_))
    assert abs(theta / w[0] - 1) < 1e-12, (label, theta, w[0])
    assert numpy.abs(v - u).max() < 1e-10, (label, cm.eigen_matvecs_, cm.eigen_residual_)
    assert abs(numpy.linalg.norm(v) - 1) < 1e-13 and v[numpy.argmax(numpy.abs(v))] > 0
    assert res <= 10 * TOL * abs(theta), (label, res, theta)
    assert cm.is_resident


@pytest.mark.parametrize("family", ["hic", "neg"])
@pytest.mark.parametrize("d", [4095, 4096, 4097, 8193])
def test_eigenvector_at_the_two_stage_switch(d, family):
    m = lm.EIGEN_FAMILIES[family](d)
    cm = bb.ContactMap.from_matrix(m)
    v = cm.eigenvector()
    check_eigenpair(cm, v, m, "d=%d %s" % (d, family))


@pytest.mark.parametrize("family", ["hic", "neg"])
@pytest.mark.parametrize("d", [4095, 4097])
def test_eigenvector_reported_residual_is_the_residual(d, family):
    """A run cut short while its residual is still >= 1e-8 |theta|: the reported
    `eigen_residual_` (|beta_n y_n| of the Lanczos relation) agrees with the long-double residual
    of the returned pair within 1e-6 relative -- the relation holds to 1e-14 |theta| -- and the
    returned eigenvalue is the pair's Rayleigh quotient to 1e-12 relative.  A dot or a beta that
    is off shows here at once: the estimate is made of them."""
    m = lm.EIGEN_FAMILIES[family](d)
    cm = bb.ContactMap.from_matrix(m)
    found = None
    for budget in (20, 16, 12, 8, 6, 4, 3, 2):
        try:
            cm.eigenvector(max_matvecs=budget)
            continue                                   # converged: nothing cut short
        except bb.EigenNoConvergence as err:
            theta, v = err.eigenvalue, err.eigenvector
        res, rayleigh = lm.residual_longdouble(m, theta, v)
        print("d=%d %s, %d products: reported %.6e, long-double %.6e (%.2e |theta|), eigenvalue "
              "against Rayleigh quotient %.2e" % (d, family, budget, cm.eigen_residual_, res,
                                                  res / abs(theta), abs(theta / rayleigh - 1)))
        if res >= 1e-8 * abs(theta):
            found = budget
            break
    assert found is not None, "no cut-short run with a residual >= 1e-8 |theta|"
    assert cm.eigen_matvecs_ == found and theta == cm.eigenvalue_
    assert abs(cm.eigen_residual_ / res - 1) < 1e-6, (cm.eigen_residual_, res)
    assert abs(theta / rayleigh - 1) < 1e-12, (theta, rayleigh)
    assert abs(numpy.linalg.norm(v) - 1) < 1e-13 and v[numpy.argmax(numpy.abs(v))] > 0


@pytest.mark.parametrize("family", ["hic", "neg"])
def test_eigenvector_same_bits_on_every_run(family):
    """The segment sums are added in a fixed order: two calls on one map and one on a fresh map
    of the same matrix give the same bits and count the same products (d = 4,097)."""
    m = lm.EIGEN_FAMILIES[family](4097)
    cm = bb.ContactMap.from_matrix(m)
    v1 = cm.eigenvector()
    n1 = cm.eigen_matvecs_
    v2 = cm.eigenvector()
    assert numpy.array_equal(bits(v1), bits(v2)) and cm.eigen_matvecs_ == n1
    fresh = bb.ContactMap.from_matrix(m.copy())
    v3 = fresh.eigenvector()
    assert numpy.array_equal(bits(v1), bits(v3)) and fresh.eigen_matvecs_ == n1
    assert fresh.eigenvalue_ == cm.eigenvalue_ and fresh.eigen_residual_ == cm.eigen_residual_


def test_eigenvector_across_filter_on_one_map():
    """4,200 bins of which 200 are dead (two-stage dots), `filter(0)` to 4,000 (one-stage dots),
    the eigenvector before and after on the same object, each against eigsh on its own host
    matrix."""
    m, dead = lm.filter_eigen_map()
    cm = bb.ContactMap.from_matrix(m)
    dev = cm._resident()
    v = cm.eigenvector()
    check_eigenpair(cm, v, m, "d=4200 with 200 dead bins")
    cm.filter(0)
    assert cm.shape == (4000, 4000) and cm._resident() is dev
    live = numpy.setdiff1d(numpy.arange(4200), dead)
    mf = numpy.ascontiguousarray(m[numpy.ix_(live, live)])
    vf = cm.eigenvector()
    check_eigenpair(cm, vf, mf, "d=4000 after filter")


# ---- 3. correlation on every center_rows_reg_kernel<CH> ----------------------------------------
def check_correlation(got, want, label):
    """The assertions of test_contactmap_correlation_vs_numpy."""
    err = numpy.abs(got - want).max()
    print("%s: max |got - numpy.corrcoef| %.2e, diagonal %.1e" %
          (label, err, numpy.abs(numpy.diag(got) - 1).max()))
    assert got.shape == want.shape
    assert err < 1e-10, (label, err)
    assert lm.is_symmetric_bitwise(got)                        # mirrored, not recomputed
    assert numpy.abs(numpy.diag(got) - 1).max() < 1e-12


@pytest.mark.parametrize("d", [2047, 2048,        # either side of the switch from center_rows_kernel
                               4097,              # CH = 8, smallest
                               8185, 8192,        # CH = 8, ldx = 8192: padding to the last lane / none
                               8193])             # CH = 16, smallest
def test_correlation_vs_numpy_full(d):
    m = lm.corr_matrix(d)
    cm = bb.ContactMap.from_matrix(m)
    assert cm.correlation() is None and cm.is_resident
    check_correlation(cm.to_host(), numpy.corrcoef(m), "d=%d" % d)
    if d == 4097:
        m[3, :] = 7.0                                          # zero variance: 0 / 0
        cm2 = bb.ContactMap.from_matrix(m)
        cm2.correlation()
        with numpy.errstate(all="ignore"):
            want2 = numpy.corrcoef(m)
        got2 = cm2.to_host()
        assert numpy.array_equal(numpy.isnan(got2), numpy.isnan(want2))
        assert numpy.isnan(want2[3]).all() and numpy.isnan(want2[:, 3]).all()
        ok = ~numpy.isnan(want2)
        assert numpy.abs(got2[ok] - want2[ok]).max() < 1e-10


@pytest.mark.parametrize("d", [16385,             # CH = 24, smallest
                               24577])            # CH = 32, smallest
def test_correlation_vs_numpy_sampled_rows(d):
    """A full corrcoef costs tens of seconds here: the reference is corrcoef's formula on 31
    rows (both ends, the block edges, 20 random ones) against ALL columns, and the symmetry of
    the whole result carries those rows' columns with it.  One host matrix throughout: drawn,
    uploaded, centred in place for the reference, then overwritten by the download."""
    t0 = time.time()
    m = lm.cheap_symmetric(d)
    t1 = time.time()
    cm = bb.ContactMap.from_matrix(m)
    dev = cm._resident()
    cm.correlation()
    t2 = time.time()
    rows = lm.sample_rows(d)
    want = lm.corrcoef_rows(m, rows, in_place=True)
    t3 = time.time()
    _lib.check(dev._lib.bb_cm_download(dev._h, _lib.as_f64_ptr(m), d), "bb_cm_download")
    got = m
    t4 = time.time()
    err = numpy.abs(got[rows] - want).max()
    diag = numpy.abs(numpy.diag(got) - 1).max()
    sym = lm.is_symmetric_bitwise(got)
    print("d=%d: max |got - reference| on %d rows %.2e, diagonal %.1e; draw %.1f s, upload + "
          "correlation %.1f s, reference %.1f s, download %.1f s, checks %.1f s"
          % (d, rows.shape[0], err, diag, t1 - t0, t2 - t1, t3 - t2, t4 - t3, time.time() - t4))
    assert err < 1e-10, (d, err)
    assert sym
    assert diag < 1e-12
    assert numpy.abs(got).max() <= 1.0                         # clipped, and no NaN anywhere


# ---- 4. small after large on the shared scratch ------------------------------------------------
def test_small_calls_after_a_large_one_on_the_shared_scratch():
    """The per-device scratch only grows, and correlation and shortest paths share it.  After a
    correlation at d = 8,193 has filled it, a correlation at d = 300 (the path that clears its
    centred rows with one memset), one at d = 2,049 (only the padding rows are cleared, the
    kernel stores each row's own padding) and a shortest-path completion of a 513-bin map must
    give the bits they give on a fresh scratch: nothing is read that the call did not write."""
    lib = _lib.load()
    a300, a2049, c513 = lm.corr_matrix(300), lm.corr_matrix(2049), lm.hic_like_counts(513, 513)

    def small_calls():
        out = []
        for a in (a300, a2049):
            cm = bb.ContactMap.from_matrix(a)
            cm.correlation()
            out.append(cm.to_host())
        sp = bb.ContactMap.from_matrix(c513).shortest_paths()
        out.append(sp.to_host())
        return out, sp.unreachable_pairs_

    assert lib.bb_cm_release_scratch(0) == _lib.BB_OK
    big = bb.ContactMap.from_matrix(lm.cheap_symmetric(8193))
    big.correlation()
    assert numpy.abs(numpy.diag(big.to_host()) - 1).max() < 1e-12     # it ran
    del big
    dirty, dirty_unreachable = small_calls()
    assert lib.bb_cm_release_scratch(0) == _lib.BB_OK
    clean, clean_unreachable = small_calls()
    for name, a, b in zip(("correlation d=300", "correlation d=2049", "shortest paths d=513"),
                          dirty, clean):
        differ = int((bits(a) != bits(b)).sum())
        assert differ == 0, (name, differ)
    assert dirty_unreachable == clean_unreachable
    # and they are answers, not two copies of the same garbage
    assert numpy.abs(clean[0] - numpy.corrcoef(a300)).max() < 1e-10
    assert numpy.abs(clean[1] - numpy.corrcoef(a2049)).max() < 1e-10
