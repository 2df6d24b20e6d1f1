"""CPU: the one-partner maps and the longdouble pair model that tests/test_gpu_pair_math.py holds
the solver's pair arithmetic to (tests/_pair_model.py).  Asserted here, not assumed there: the
matching is one, it reaches every combination of the pair steps' template arguments on every unit
layout, every operand class meets every position class, the operands are dtype values with the
stated geometry, and the longdouble formula agrees with mpmath at 50 digits."""
import numpy
import pytest

from tests import _pair_model as pm

pytestmark = pytest.mark.skipif(not pm.HAVE_LONGDOUBLE, reason=pm.LONGDOUBLE_REASON)

SWEEPS = sorted(pm.SWEEP_SIZES.items())
ROW_OWNERS = [(d, n) for d, sizes in sorted(pm.ROW_OWNER_SIZES.items()) for n in sizes]
ALL_SIZES = sorted({n for _, n in SWEEPS} | {n for _, n in ROW_OWNERS})


@pytest.mark.parametrize("n", ALL_SIZES)
def test_every_bin_has_one_partner(n):
    i, j, off, lonely = pm.matching(n)
    assert (i < j).all() and numpy.array_equal(j - i, off)
    assert set(off.tolist()) <= set(pm.OFFSETS) == {1, 2, 3, 5, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1031}
    seen = numpy.concatenate([i, j, numpy.asarray(lonely, dtype=numpy.int64)])
    assert numpy.array_equal(numpy.sort(seen), numpy.arange(n))
    assert lonely == ([n - 1] if n % 2 else [])


@pytest.mark.parametrize("layout,n", SWEEPS)
def test_matching_reaches_every_position_of_the_unit_sweep(layout, n):
    """Every (matrix row of the unit, load of the lane, column of the load) -- K, H, R and the half of
    a scalar pair in pair_step2, C and the row in pair_step --, 32 lanes or more, and tiles on and
    off the diagonal."""
    i, j, off, _ = pm.matching(n)
    lay = pm.LAYOUTS[layout]
    pos = pm.positions(layout, i, j)
    rows = {"f32": 4, "f64n": 8, "f64w": 2}[layout]
    loads = {"f32": 2, "f64n": 1, "f64w": 4}[layout]
    cols = {"f32": 4, "f64n": 2, "f64w": 2}[layout]
    assert (lay["rows_per_unit"], lay["cols"]) == (rows, cols)
    combos = set(zip(pos["row"].tolist(), pos["load"].tolist(), pos["col"].tolist()))
    assert combos == {(r, k, c) for r in range(rows) for k in range(loads) for c in range(cols)}
    cls, n_cls = pm.position_class(layout, i, j)
    assert n_cls == rows * loads * cols and set(cls.tolist()) == set(range(n_cls))
    assert len(set(pos["lane"].tolist())) >= 32
    assert pos["diag"].any() and (~pos["diag"]).any()
    if layout == "f32":      # both halves of every scalar pair of XRowS32: coordinate q = 3 r + c
        assert {(3 * r + c) & 1 for r in set(pos["row"].tolist()) for c in range(3)} == {0, 1}
    print("%s N = %d: %d pairs, offsets %s, %d lanes" % (layout, n, i.size, sorted(set(off.tolist())),
                                                         len(set(pos["lane"].tolist()))))


@pytest.mark.parametrize("layout,n", SWEEPS)
def test_every_operand_class_meets_every_position_of_the_unit_sweep(layout, n):
    dtype = pm.LAYOUTS[layout]["dtype"]
    for e in pm.SCALES[dtype]:
        case = pm.operands(n, dtype, e, q=0, layout=layout)
        cls, n_cls = pm.position_class(layout, case.i, case.j)
        want = set(range(n_cls))
        for name in pm.DIRECTIONS:
            assert {c for c, d in zip(cls.tolist(), case.direction) if d == name} == want, (e, name)
        for name, _ in pm.ratios(dtype):
            assert {c for c, r in zip(cls.tolist(), case.ratio) if r == name} == want, (e, name)
        assert pm.EXACT in case.ratio
        assert (pm.FLOOR in case.ratio) == (e == 0)


@pytest.mark.parametrize("dtype,n", ROW_OWNERS)
def test_every_operand_class_meets_every_column_of_a_row_owner_trip(dtype, n):
    for e in pm.SCALES[dtype]:
        for q in (0, 1, 2):
            case = pm.operands(n, dtype, e, q=q)
            at_j, at_i, cols = pm.row_owner_class(dtype, case.i, case.j)
            want = set(range(cols))
            for name in pm.DIRECTIONS:
                k = [d == name for d in case.direction]
                assert set(at_j[k].tolist()) == want and set(at_i[k].tolist()) == want, (e, q, name)
            for name, _ in pm.ratios(dtype):
                k = [r == name for r in case.ratio]
                assert set(at_j[k].tolist()) == want and set(at_i[k].tolist()) == want, (e, q, name)
            assert pm.EXACT in case.ratio and (pm.FLOOR in case.ratio) == (e == 0 and q == 0)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("q", [0, 1, 2])
def test_operands_are_dtype_values_with_the_stated_geometry(dtype, q):
    T = pm.np_dtype(dtype)
    n = pm.ROW_OWNER_SIZES[dtype][0]
    for e in pm.SCALES[dtype]:
        case = pm.operands(n, dtype, e, q=q)
        assert numpy.array_equal(case.x.astype(T).astype(numpy.float64), case.x)
        assert numpy.array_equal(case.delta.astype(T).astype(numpy.float64), case.delta)
        ref = pm.reference(case, q)
        scale = pm.LD(2) ** e
        assert (ref.d >= scale / 4).all() and (ref.d <= scale * 5 / 8 * (1 + pm.LD(2) ** -20)).all()
        xi, xj = case.x[case.i].astype(pm.LD), case.x[case.j].astype(pm.LD)
        c, v = (xi + xj) / 2, (xi - xj) / 2
        assert ((c * c).sum(1) <= (v * v).sum(1)).all()               # about its own midpoint
        dx = numpy.abs(xi - xj)
        for a, name in enumerate(case.direction):
            if name in ("x", "y", "z"):                                 # the other products are exact zeros
                assert numpy.count_nonzero(dx[a]) == 1 and dx[a]["xyz".index(name)] > 0
            if name == "111":
                assert dx[a][0] == dx[a][1] == dx[a][2] > 0
            if name == "122":
                assert 2 * dx[a][0] == dx[a][1] == dx[a][2] > 0
        tol = 2 * float(pm.U[dtype])
        for a, (rname, rval) in enumerate(pm.ratios(dtype)):
            k = numpy.asarray([r == rname for r in case.ratio])
            assert k.any() and (numpy.abs(case.delta[k].astype(pm.LD) / ref.d[k] / rval - 1) <= tol).all()
        k = numpy.asarray([r == pm.EXACT for r in case.ratio])
        assert k.any() and all(case.direction[a] == "122" for a in numpy.flatnonzero(k))
        assert numpy.array_equal(case.delta[k], ref.d[k].astype(T).astype(numpy.float64))
        # the wish distances survive the flush of SPEC 2.1 and every weighted term is finite
        assert (case.delta >= pm.WISH_FLOOR[dtype]).all()
        assert ((pm.FLOOR in case.ratio) == (e == 0 and q == 0))
        big = pm.LD(numpy.finfo(T).max)
        assert ref.s.sum() < big / 4 and numpy.abs(ref.g).max() < big / 4
        assert (case.delta.astype(pm.LD) ** max(q, 1) >= pm.LD(numpy.finfo(T).tiny)).all()


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_longdouble_model_against_mpmath(dtype):
    """Every operand class, every scale and weight power: the longdouble g_i and stress term within
    2^-60 of the (d + delta) form of the 50-digit value."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    n = 129 if dtype == "float64" else 513
    tol = mp.mpf(2) ** -60

    def big(v):                                  # a float64 value: exact
        return mp.mpf(float(v))

    def of_ld(v):                                # a longdouble as the sum of two doubles: exact
        hi = float(v)
        return mp.mpf(hi) + mp.mpf(float(v - pm.LD(hi)))

    worst = mp.mpf(0)
    seen = set()
    for e in pm.SCALES[dtype]:
        for q in (0, 1, 2):
            case = pm.operands(n, dtype, e, q=q)
            ref = pm.reference(case, q)
            eps2 = of_ld(pm.eps2(dtype))
            for a in range(case.i.size):
                seen.add((case.direction[a], case.ratio[a]))
                dx = [big(case.x[case.i[a], c]) - big(case.x[case.j[a], c]) for c in range(3)]
                delta = big(case.delta[a])
                d = mp.sqrt(dx[0] ** 2 + dx[1] ** 2 + dx[2] ** 2 + eps2)
                w = delta ** (-q)
                for c in range(3):
                    unit = 2 * abs(dx[c]) * (d + delta) / d * w
                    err = abs(of_ld(ref.g[a, c]) - 2 * (d - delta) / d * w * dx[c])
                    assert err <= tol * unit, (e, q, a, c)
                    if unit > 0:
                        worst = max(worst, err / unit)
                    assert abs(of_ld(ref.unit_g[a, c]) - unit) <= tol * unit
                unit = (d + delta) ** 2 * w
                err = abs(of_ld(ref.s[a]) - (d - delta) ** 2 * w)
                assert err <= tol * unit, (e, q, a)
                worst = max(worst, err / unit)
                assert abs(of_ld(ref.unit_s[a]) - unit) <= tol * unit
    assert {d for d, _ in seen} == set(pm.DIRECTIONS)
    assert {r for _, r in seen} >= {r for r, _ in pm.ratios(dtype)} | {pm.EXACT, pm.FLOOR}
    print("%s: longdouble against mpmath, worst %.3g of 2^-60" % (dtype, float(worst / tol)))


def test_counts():
    """C and C_S are twice the counted roundings, for every copy and weight power a test uses."""
    for copy, per_q in pm.COUNTS.items():
        for q, (g, s) in per_q.items():
            assert pm.bound_factors(copy, q) == (2 * g, 2 * s) and g >= 9 and s >= 9
    assert pm.COUNTS["f64 sweep"] == pm.COUNTS["f64 row owner"]      # one expression (pair_step, pair_row)
