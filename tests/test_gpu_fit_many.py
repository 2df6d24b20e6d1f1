"""GPU: several maps in one solver (StructureSolver.fit_many, bb_solver_set_maps) at every map-size
edge, weight power and step rule.  Three rules hold only across a map boundary -- a wave's stress
partial belongs to the strip (and so the map) the wave ENDS in and every strip it left has a slot
of its own; a map's step reaches the update through the per-bin factors alone; the rows between
the maps never move and no map's numbers reach another's -- so every map is held against the
oracle's run of that map alone (tests/_many_model.py: Hi-C-like count maps with dead bins, missing
pairs and NaN / inf entries, map m at 2^(m % 7) times the scale of map 0, so that a partial put to
the wrong map cannot hide in the tolerance).  Tolerances: fp64 1e-12, fp32 1e-5, relative, on
every entry of a map's stress history and on its max-abs coordinates (below 16 bins the stress
against the start's: `_many_model.errors`)."""
import numpy
import pytest

import blueberry_amd as bb
from blueberry_amd.solver import HipEngine
from tests import _many_model as mm
from tests import _oracle
from tests.test_gpu_contactmap_stage import cu_count
from tests.test_weighted_stress import start, wish_of

pytestmark = pytest.mark.gpu

DTYPES = ["float64", "float32"]
PLAIN, SAMMON, RELATIVE = mm.Setting(0, 0.0, False), mm.Setting(1, 0.0, False), mm.Setting(2, 0.0, False)
EDGE_SETTINGS = {"plain": PLAIN, "momentum": mm.Setting(0, 0.3, False), "q1": SAMMON, "q2": RELATIVE}


def _solver(dtype, setting, k, **more):
    return bb.StructureSolver(n_iter=k, dtype=dtype, kind="counts", momentum=setting.mu,
                              weight_power=setting.q, degree_steps=setting.degree_steps, **more)


def _check_maps(b, dtype, setting, k, structures, histories, lrs=None, what=""):
    """Every map of the batch against the oracle's run of it alone; returns the references."""
    tol = mm.TOL[dtype]
    worst_s = worst_x = 0.0
    refs = []
    for m, n in enumerate(b.sizes):
        X_ref, h_ref, lr, scale = mm.reference(b.wish[m], b.starts[m], k, setting, dtype)
        refs.append((X_ref, h_ref))
        if lrs is not None:
            assert abs(lrs[m] / lr - 1) <= mm.step_bound(b.wish[m], setting, dtype), (m, n, lrs[m], lr)
        assert numpy.isfinite(histories[m]).all() and numpy.isfinite(structures[m]).all(), (m, n)
        err_s, err_x = mm.errors(n, structures[m], histories[m], X_ref, h_ref)
        worst_s, worst_x = max(worst_s, err_s), max(worst_x, err_x)
        assert err_s < tol and err_x < tol, (m, n, dtype, setting, err_s, err_x)
    print("%s %s q=%d mu=%.1f degree_steps=%d: %d maps, %d bins: worst stress %.2e coords %.2e"
          % (what, dtype, setting.q, setting.mu, setting.degree_steps, len(b.sizes), sum(b.sizes),
             worst_s, worst_x))
    return refs


# ---- 1. size edges ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(EDGE_SETTINGS))
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("batch", list(mm.SIZE_EDGES))
def test_fit_many_size_edges(batch, dtype, name):
    """Maps of 2 bins and maps of thousands, maps that end on a tile edge so that the next one
    abuts, many maps, a map per block, fp64 batches on both sides of the 128- / 512-wide switch."""
    setting, k = EDGE_SETTINGS[name], 4
    b = mm.batch(mm.SIZE_EDGES[batch], 1, dtype)
    s = _solver(dtype, setting, k).fit_many(list(b.counts), inits=list(b.starts))
    assert s.n_bins_many_ == list(b.sizes) and s.n_iter_ == k
    assert len(s.structures_) == len(s.stresses_) == len(s.lrs_) == len(b.sizes)
    _check_maps(b, dtype, setting, k, s.structures_, s.stresses_, s.lrs_, "size edges " + batch)


@pytest.mark.parametrize("dtype", DTYPES)
def test_fit_many_spectral_starts_map_by_map(dtype):
    """init='spectral': every map starts where its single fit(init='spectral') does (maps under 4
    bins through the host form), and goes on as that fit does.  A map of 2 bins starts AT its wish
    distance and one of a few bins next to them: the start's stress is 0 or rounding noise, so
    below 16 bins a history that starts under a thousandth of the collapsed structure's stress,
    the sum of delta^2 (`_many_model.collapsed_stress`), is compared on that scale; the other
    small maps against their start's stress and the maps from 16 bins on entry by entry."""
    k, tol = 2, mm.TOL[dtype]
    b = mm.batch(mm.SPECTRAL, 4, dtype)
    s = _solver(dtype, PLAIN, k, init="spectral").fit_many(list(b.counts))
    at0 = _solver(dtype, PLAIN, 0, init="spectral").fit_many(list(b.counts))
    assert at0.n_iter_ == 0
    for m, n in enumerate(b.sizes):
        collapsed = mm.collapsed_stress(b.wish[m])
        assert collapsed > 0
        one0 = _solver(dtype, PLAIN, 0, init="spectral").fit(b.counts[m])
        one = _solver(dtype, PLAIN, k, init="spectral").fit(b.counts[m])
        assert at0.structures_[m].shape == (n, 3) and at0.stresses_[m].shape == (0,)
        err_0 = mm.errors(n, at0.structures_[m], at0.stresses_[m], one0.structure_, one0.stress_)[1]
        scale = one.stress_[0] if one.stress_[0] > 1e-3 * collapsed else collapsed
        err_s, err_x = mm.errors(n, s.structures_[m], s.stresses_[m], one.structure_, one.stress_, scale)
        print("spectral %s n=%d: start %.2e, after %d steps stress %.2e coords %.2e (first stress %.2e "
              "of the collapsed structure's)" % (dtype, n, err_0, k, err_s, err_x, one.stress_[0] / collapsed))
        assert err_0 < tol and err_s < tol and err_x < tol, (m, n, err_0, err_s, err_x)
        # the start is the map's classical-MDS solution, not the seeded normal one
        assert not numpy.array_equal(at0.structures_[m],
                                     numpy.random.default_rng(0).standard_normal((n, 3)))
        # and the steps from there are the oracle's
        X_ref, h_ref, _, _ = mm.reference(b.wish[m], at0.structures_[m], k, PLAIN, dtype)
        err_s, err_x = mm.errors(n, s.structures_[m], s.stresses_[m], X_ref, h_ref, scale)
        assert err_s < tol and err_x < tol, (m, n, err_s, err_x)


# ---- engine level -----------------------------------------------------------------------------------
class _Run(object):
    """A batch in an engine of its own, as `_fit_many_local` lays it out: kind='wish' from the
    batch's wish maps, so the device holds the model's matrix to the bit."""

    def __init__(self, b, dtype, setting, lr_scale=None):
        self.b, self.dtype, self.lay = b, dtype, mm.joint_layout(b.sizes, dtype)
        lay = self.lay
        self.eng = eng = HipEngine(lay["total"], dtype, tiles=lay["tiles"])
        try:
            assert eng.layout()["n_units"] == lay["n_units"]
            per = [mm.steps(w, setting) for w in b.wish]
            # the maps' steps through set_maps (lr_scale: one per map) or through set_bin_steps
            eng.set_maps(lay["off"] + [lay["total"]],
                         [1.0] * len(b.sizes) if lr_scale is None else lr_scale)
            x0 = numpy.zeros((lay["total"], 3))
            steps = numpy.ones(lay["total"])
            self.inside = numpy.zeros(lay["total"], dtype=bool)
            for o, n, w, x, (lr, scale) in zip(lay["off"], b.sizes, b.wish, b.starts, per):
                eng.set_wish_dense_block(w, o, "wish", 3.0)
                x0[o:o + n] = x
                steps[o:o + n] = lr if scale is None else lr * scale
                self.inside[o:o + n] = True
            if setting.q:
                eng.set_weight_power(setting.q)
            if lr_scale is None:
                eng.set_bin_steps(steps)
            eng.set_coords(x0)
            if setting.mu:
                eng.set_momentum(setting.mu)
        except BaseException:
            eng.close()
            raise

    def split(self, X):
        return [X[o:o + n] for o, n in zip(self.lay["off"], self.b.sizes)]

    def close(self):
        self.eng.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("batch", ["narrow_edges", "two_bins_between"])
def test_padding_rows_between_the_maps_never_move(batch, dtype):
    setting, k = mm.Setting(2, 0.3, True), 4
    b = mm.batch(mm.SIZE_EDGES[batch], 1, dtype)
    run = _Run(b, dtype, setting)
    try:
        assert (~run.inside).sum() > 0
        run.eng.iterate(k, 1.0)
        X = run.eng.get_coords()
        hist = run.eng.stress_history().reshape(k, len(b.sizes))
    finally:
        run.close()
    assert not X[~run.inside].any()
    _check_maps(b, dtype, setting, k, run.split(X), list(hist.T), what="padding " + batch)


# ---- 2. a genome at 1 Mb ----------------------------------------------------------------------------
@pytest.mark.parametrize("degree_steps", [False, True])
@pytest.mark.parametrize("q", [0, 1, 2])
@pytest.mark.parametrize("dtype", DTYPES)
def test_fit_many_genome_at_1mb(dtype, q, degree_steps):
    """The 23 maps of chr1 .. chrX at 1 Mb (49 to 250 bins: every map smaller than a tile), each
    with its own step and, with degree_steps, its own per-bin factors: against the oracle and
    against the single fit(), while waves hold units of two maps."""
    setting, k = mm.Setting(q, 0.0, degree_steps), 6
    b = mm.batch(mm.GENOME_1MB, 2, dtype)
    lay = mm.joint_layout(b.sizes, dtype)
    cus = cu_count()
    wpc, wpb = mm.launch_shape(lay["n_units"], dtype, lay["vw"], cus)
    plan = mm.wave_plan(lay["n_units"], lay["units_per_tile"], lay["tile_map"], cus, wpc, wpb)
    assert mm.crossing(plan)[0] >= 1
    s = _solver(dtype, setting, k).fit_many(list(b.counts), inits=list(b.starts))
    assert s.n_bins_many_ == list(b.sizes) and s.n_iter_ == k
    _check_maps(b, dtype, setting, k, s.structures_, s.stresses_, s.lrs_, "genome at 1 Mb")
    for m, n in enumerate(b.sizes):
        if degree_steps and q == 0:
            assert s.lrs_[m] == mm.steps(b.wish[m], setting)[0]        # integers: exact
        one = _solver(dtype, setting, k).fit(b.counts[m], init=b.starts[m])
        # (the single fit sums its weighted degrees over another layout: both within the bound)
        assert abs(s.lrs_[m] / one.lr_ - 1) <= 2 * mm.step_bound(b.wish[m], setting, dtype)
        err_s, err_x = mm.errors(n, s.structures_[m], s.stresses_[m], one.structure_, one.stress_)
        assert err_s < mm.TOL[dtype] and err_x < mm.TOL[dtype], (m, n, err_s, err_x)


# ---- 3. waves that pass through whole maps ------------------------------------------------------------
@pytest.mark.parametrize("q", [0, 2])
@pytest.mark.parametrize("dtype", DTYPES)
def test_waves_that_pass_through_whole_maps(dtype, q, monkeypatch):
    """311 single-tile maps under one wave per CU: a wave's chunk is longer than a tile, so waves
    leave a map behind mid-sweep (its stress goes out through a private slot) and some hold the
    end of one map, all of the next and the start of a third."""
    monkeypatch.setenv("BB_WAVES_PER_CU", "1")
    setting, k = mm.Setting(q, 0.0, False), 3
    b = mm.batch(mm.THROUGH, 3, dtype)
    nm = len(b.sizes)
    lay = mm.joint_layout(b.sizes, dtype)
    assert lay["vw"] == 512 and lay["units_per_tile"] == (128 if dtype == "float32" else 256)
    cus = cu_count()
    wpc, wpb = mm.launch_shape(lay["n_units"], dtype, lay["vw"], cus, 1)
    plan = mm.wave_plan(lay["n_units"], lay["units_per_tile"], lay["tile_map"], cus, wpc, wpb)
    two, most, _ = mm.crossing(plan)
    assert most >= 3 and 4 * two >= len(plan), (two, most, len(plan))
    o = _oracle.load()
    run = _Run(b, dtype, setting)
    try:
        per = run.eng.stress_maps()
        whole = run.eng.stress()
        run.eng.iterate(k, 1.0)
        X = run.eng.get_coords()
        hist = run.eng.stress_history()
    finally:
        run.close()
    assert per.shape == (nm,) and hist.shape == (k * nm,)
    assert abs(per.sum() / whole - 1) < 1e-12
    hist = hist.reshape(k, nm)
    refs = _check_maps(b, dtype, setting, k, run.split(X), list(hist.T),
                       what="through whole maps (%d of %d waves cross, up to %d maps)" % (two, len(plan), most))
    worst = 0.0
    for m, n in enumerate(b.sizes):
        s0, _ = o.stress_grad_weighted(b.wish[m], b.starts[m], q, f64=dtype == "float64")
        assert s0 == refs[m][1][0]
        worst = max(worst, abs(per[m] / s0 - 1))
        assert abs(per[m] / s0 - 1) < mm.TOL[dtype], (m, n, per[m], s0)
    assert not X[~run.inside].any()
    print("through whole maps %s q=%d: stress_maps before the first step, worst %.2e" % (dtype, q, worst))


# ---- 4. maps do not reach each other --------------------------------------------------------------------
def _isolation_run(b, dtype, setting, k, lr_scale):
    run = _Run(b, dtype, setting, lr_scale=lr_scale)
    try:
        run.eng.iterate(k, 1.0)
        return run.split(run.eng.get_coords()), run.eng.stress_history().reshape(k, len(b.sizes))
    finally:
        run.close()


@pytest.mark.parametrize("q", [0, 2])
@pytest.mark.parametrize("layout", sorted(mm.ISOLATION))
def test_maps_do_not_reach_each_other(layout, q):
    """Two runs that differ in map 2 alone -- other data of the same size, then a step so large
    that the map's stress leaves the finite numbers -- leave every other map's coordinates and
    stress history bit for bit the same: no tile joins two maps, a block's reduce list holds its
    own chunks alone, and a map's stress is folded from its own partials.  Maps 0 | 1 and 2 | 3
    abut without a padding row."""
    dtype, sizes = mm.ISOLATION[layout]
    setting, k, odd = mm.Setting(q, 0.0, False), 4, 2
    b = mm.batch(sizes, 6, dtype)
    lay = mm.joint_layout(sizes, dtype)
    assert lay["vw"] == (128 if layout == "fp64_narrow" else 512)
    lrs = [mm.steps(w, setting)[0] for w in b.wish]
    base_X, base_h = _isolation_run(b, dtype, setting, k, lrs)
    _check_maps(b, dtype, setting, k, base_X, list(base_h.T), what="isolation " + layout)
    # the same batch with another map 2
    w2 = wish_of(mm.counts_of(sizes[odd], 999, odd), dtype)
    assert w2.shape == b.wish[odd].shape and not numpy.array_equal(w2, b.wish[odd])
    other = mm.Batch(b.sizes, b.counts, b.wish[:odd] + (w2,) + b.wish[odd + 1:],
                     b.starts[:odd] + (start(sizes[odd], w2, seed=998),) + b.starts[odd + 1:])
    lrs_other = list(lrs)
    lrs_other[odd] = mm.steps(w2, setting)[0]
    other_X, other_h = _isolation_run(other, dtype, setting, k, lrs_other)
    # ... and with a step that throws map 2 out of the finite numbers
    wild = list(lrs)
    wild[odd] = lrs[odd] * (1e30 if dtype == "float32" else 1e200)
    wild_X, wild_h = _isolation_run(b, dtype, setting, k, wild)
    assert not numpy.isfinite(wild_h[:, odd]).all()
    assert not numpy.array_equal(other_h[:, odd], base_h[:, odd])
    for m in range(len(sizes)):
        if m == odd:
            continue
        for X, h, what in ((other_X, other_h, "other data"), (wild_X, wild_h, "diverging step")):
            assert numpy.isfinite(h[:, m]).all() and numpy.isfinite(X[m]).all(), (m, what)
            assert numpy.array_equal(h[:, m], base_h[:, m]), (m, what)
            assert numpy.array_equal(X[m], base_X[m]), (m, what)


# ---- 5. history capacity ------------------------------------------------------------------------------------
def test_stress_history_capacity_with_23_maps():
    """The history holds 2^20 values, n_maps per iteration: a call that would pass that is refused
    whole (the largest that fits, 45,590 iterations, is not run here)."""
    dtype, nm = "float32", len(mm.HISTORY)
    most = mm.HIST_CAP // nm
    b = mm.batch(mm.HISTORY, 8, dtype)
    run = _Run(b, dtype, PLAIN)
    try:
        with pytest.raises(RuntimeError, match="stress history full"):
            run.eng.iterate(most + 1, 1.0)
        assert run.eng.stress_history().shape == (0,)
        run.eng.iterate(2, 1.0)
        X = run.eng.get_coords()
        hist = run.eng.stress_history()
        assert hist.shape == (2 * nm,)
        with pytest.raises(RuntimeError, match="stress history full"):
            run.eng.iterate(most - 1, 1.0)
        assert numpy.array_equal(run.eng.stress_history(), hist)
        assert numpy.array_equal(run.eng.get_coords(), X)
        run.eng.iterate(1, 1.0)                                   # and it still iterates
        assert run.eng.stress_history().shape == (3 * nm,)
    finally:
        run.close()
