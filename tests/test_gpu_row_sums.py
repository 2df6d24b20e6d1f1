"""GPU: the row side of the fp32 unit sweep.  A unit's 12 row sums (4 matrix rows x 3 components)
leave the wave through one transposed lane reduction and one store or one LDS parking slot per
unit (bb_solver_kernels.h, process_unit_f32).  What must hold whatever the tree looks like:

  - two runs of the same fit give the same bits, coordinates and stress history;
  - a unit's row sums do not depend on whether the wave parked them in LDS or stored them
    directly, nor on which wave swept the unit;
  - the row sums of one sweep are the sums of the per-pair forces of SPEC 2.3, on a ragged size
    too, at the fp32 tolerance of the suite (1e-5, relative to the largest entry).

Row sums are looked at through a BIPARTITE tile list: tiles (I, J) with every I below every J.
The bins of the row blocks then receive nothing but row sums, the bins of the column blocks
nothing but column partials, and the gradient of a row bin is the sum of its units' row sums
in the fixed order of the reduce."""
import numpy
import pytest

from blueberry_amd.solver import HipEngine
from tests import _oracle

pytestmark = pytest.mark.gpu

VW, UPT = 512, 128            # fp32: 512-column strips, 128 units of 4 rows per tile
TOL32 = 1e-5


def _bipartite(row_blocks, col_blocks):
    """Tiles (I, J), I in row_blocks, J in col_blocks, in strip-major order (J, then I)."""
    tj, ti = numpy.meshgrid(numpy.asarray(col_blocks), numpy.asarray(row_blocks), indexing="ij")
    return ti.ravel().astype(numpy.int32), tj.ravel().astype(numpy.int32)


def _gradient(eng, n):
    eng.grad()
    eng.sync()
    host = eng.read_exchange()
    return host[:3 * n].reshape(n, 3).copy(), float(host[-2]) + float(host[-1])


def pair_force_sums(W, X, rows, cols):
    """Gradient of SPEC 2.3's stress over the pairs rows x cols with respect to the row bins, as a
    plain numpy sum of per-pair forces: g_i = 2 sum_j (d_ij - delta_ij) / d_ij (x_i - x_j) over
    the pairs with delta_ij > 0, d_ij^2 = |x_i - x_j|^2 + eps^2; and the stress of those pairs."""
    diff = X[rows, None, :] - X[None, cols, :]
    d = numpy.sqrt((diff * diff).sum(-1) + 1e-30)
    delta = W[numpy.ix_(rows, cols)]
    res = numpy.where(delta > 0, d - delta, 0.0)
    return 2.0 * ((res / d)[:, :, None] * diff).sum(1), float((res * res).sum())


def test_two_runs_are_bit_identical(monkeypatch):
    """The reduction tree is fixed: nothing depends on which wave ran when, and not on the
    parity of the iteration (an odd and an even number of steps, run twice each)."""
    n = 5000                                       # ragged: 9 full strips + 392 columns
    xs = _oracle.random_walk(n)
    x0 = _oracle.noisy_init(xs)
    lr = 1.0 / (2.0 * n)
    for steps in (7, 8):
        got = []
        for _ in range(2):
            eng = HipEngine(n, "float32")
            try:
                eng.set_wish_from_coords(xs)
                eng.set_coords(x0)
                eng.iterate(steps, lr)
                assert eng.iteration_path() == ("units", 0)
                got.append((eng.get_coords(), eng.stress_history()))
            finally:
                eng.close()
        assert got[0][1].shape == (steps,) and numpy.isfinite(got[0][0]).all()
        assert numpy.array_equal(got[0][0], got[1][0])
        assert numpy.array_equal(got[0][1], got[1][1])
    # the same engine, the same start, again: no state of the first run leaks into the second
    eng = HipEngine(n, "float32")
    try:
        eng.set_wish_from_coords(xs)
        runs = []
        for _ in range(2):
            eng.set_coords(x0)
            eng.iterate(8, lr)
            runs.append((eng.get_coords(), eng.stress_history()))
    finally:
        eng.close()
    assert numpy.array_equal(runs[0][0], runs[1][0]) and numpy.array_equal(runs[0][1], runs[1][1])
    assert numpy.array_equal(runs[0][0], got[0][0])


def test_parked_and_directly_stored_units_give_the_same_row_sums(monkeypatch):
    """32 row blocks x 64 column blocks = 262,144 units.  With one wave per CU a wave's chunk
    (about 1,024 units) is longer than its LDS parking space (831 units), so the first units of
    every chunk are stored directly and the rest parked; with the default 8 waves per CU (chunks
    of 128 units, 8 waves per workgroup) every unit is parked.  The row bins' gradient -- row
    sums only -- must be the same bits either way; the column bins' partials are cut differently
    and agree to rounding."""
    rows_b, cols_b = 32, 64
    n = (rows_b + cols_b) * VW - 152               # ragged last column strip
    tiles = _bipartite(range(rows_b), range(rows_b, rows_b + cols_b))
    xs = _oracle.random_walk(n)
    x0 = _oracle.noisy_init(xs)
    res = {}
    for name, env in (("parked", {}), ("mixed", {"BB_WAVES_PER_CU": "1"}),
                      ("mixed4", {"BB_WAVES_PER_CU": "4", "BB_PAIR": "0"})):
        monkeypatch.delenv("BB_WAVES_PER_CU", raising=False)
        monkeypatch.delenv("BB_PAIR", raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        eng = HipEngine(n, "float32", tiles=tiles)
        try:
            assert eng.layout()["n_units"] == rows_b * cols_b * UPT
            eng.set_wish_from_coords(xs)
            eng.set_coords(x0)
            res[name] = _gradient(eng, n)
        finally:
            eng.close()
    nr = rows_b * VW
    g_ref, s_ref = res["parked"]
    assert numpy.abs(g_ref[:nr]).max() > 0 and numpy.isfinite(g_ref).all()
    for name in ("mixed", "mixed4"):
        g, s = res[name]
        assert numpy.array_equal(g[:nr], g_ref[:nr]), name
        assert numpy.abs(g[nr:] - g_ref[nr:]).max() < TOL32 * numpy.abs(g_ref[nr:]).max()
        assert abs(s / s_ref - 1) < TOL32


@pytest.mark.parametrize("n", [3 * VW + 276, 3 * VW + 1, 4 * VW])
def test_row_sums_of_one_sweep_equal_numpy_pair_force_sums(n):
    """Row blocks {0, 1} x column blocks {2, 3}, the last strip ragged (276 columns, one column,
    or complete), a map with missing pairs.  The row bins' gradient of ONE sweep against a numpy
    sum of the per-pair forces in float64 -- pinned to the C oracle's unit sweep first."""
    tiles = _bipartite([0, 1], [2, 3])
    xs = _oracle.random_walk(n)
    x0 = _oracle.noisy_init(xs)
    W = _oracle.wish_from_coords(xs).astype(numpy.float32).astype(numpy.float64)
    rng = numpy.random.default_rng(n)
    hole = numpy.triu(rng.random((n, n)) < 0.05, 1)
    W[hole | hole.T] = 0.0                         # 5 % of the pairs carry no constraint
    W[7, :] = W[:, 7] = 0.0                        # and one row bin none at all
    rows, cols = numpy.arange(2 * VW), numpy.arange(2 * VW, n)
    g_np, s_np = pair_force_sums(W, x0, rows, cols)
    s_or, g_or = _oracle.load().stress_grad_units(W, x0, tiles[0], tiles[1], UPT, VW, 0,
                                                  len(tiles[0]) * UPT)
    assert numpy.abs(g_np - g_or[rows]).max() < 1e-12 * numpy.abs(g_or[rows]).max()
    assert abs(s_np / s_or - 1) < 1e-12
    eng = HipEngine(n, "float32", tiles=tiles)
    try:
        eng.set_wish_dense(W, "wish", 3.0)
        eng.set_coords(x0)
        g, s = _gradient(eng, n)
    finally:
        eng.close()
    err_g = float(numpy.abs(g[rows] - g_np).max() / numpy.abs(g_np).max())
    err_s = abs(s / s_np - 1)
    print("n=%d row sums vs numpy pair forces: gradient %.2e stress %.2e" % (n, err_g, err_s))
    assert not g[7].any()
    assert err_g < TOL32 and err_s < TOL32
