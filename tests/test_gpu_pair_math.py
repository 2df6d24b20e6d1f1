"""GPU: the solver's pair arithmetic, pair by pair, to a rounding bound (docs/SPEC.md 4).

d^2 = |x_i - x_j|^2 + eps^2, d, 1/d, res = d - delta, coef = res / d * delta^-q, g += coef (x_i -
x_j), S += res^2 delta^-q exist in several hand-written copies: pair_step (fp64 unit sweep, narrow and
wide), pair_step2 (fp32 unit sweep), pair_row (row owner, fp32 and fp64), each for q = 0, 1, 2.
Here every copy runs on a map whose bins have ONE partner each (tests/_pair_model.py): a masked
pair adds +-0, so the gradient of a bin is what the copy made of one pair, and it is compared with
the longdouble formula of the same dtype-rounded operands -- directions along the axes, (1, 1, 1),
(1, 2, 2) and random; delta / d from 2^-20 over 1 -+ 2^-20 (fp64: 2^-40) and delta = d to 2^20; one
engine per scale 2^e, e = -40 .. 40 (fp32) and -300 .. 300 (fp64); delta at the wish floor.

What is asserted, per copy, weight power and scale:
  1. every component of every matched bin: |g - g*| <= C u 2 |x_i - x_j|_c (d + delta) / d *
     delta^-q, u = 2^-24 / 2^-53, C = twice the roundings counted in the copy's code
     (_pair_model.COUNTS; docs/MEASUREMENTS.md, "the pair arithmetic");
  2. g_j == -g_i, bit for bit (unit sweep); on the row owner, which has no gradient read-out and
     evaluates a pair from both ends, the two updates agree to the rounding of the update alone;
  3. the lonely bin and the padding rows: exactly +0.0 (row owner: the bin does not move);
  4. |S - sum res*^2 delta^-q| <= (n + C_S) u sum (d + delta)^2 delta^-q, n the engine's pairs;
  5. path against path: pair_row<double> and pair_step<double> are one expression, so the row
     owner's new coordinates are, bit for bit, x - step * g of the fp64 sweep's gradient.  In fp32
     the row owner is a different expression from the sweep's (compares for the clamp, the
     reciprocal of delta used twice for q = 2): both are held to their own bounds, nothing more.

The row owner is read through one iterate(1, 1.0) with a step per bin (set_bin_steps) that is a
power of two and makes the move at least 2^8 times the coordinate: g~ = (x - x') / step, exact
on the host, and the rounding of x' (one ulp of it, over the step) joins that component's bound.

The two refined fp64 routines under all of this, rsqrt_sqrt_f64 and rcp_f64, are also called
directly, through a probe that build.sh compiles from the kernels' own header (tests/probes/
refined_f64_probe.hip), and held to the 2 ulp of their comments: the bound above grants each of
them those 2 ulp and then a factor 2, which alone would leave room for a routine 7 ulp off.

Scale covariance: every coordinate and wish distance times 2^e (e even) changes no significand in
SPEC 2.2 - 2.4, so K = 5 steps give 2^e times the coordinates and 2^((2 - q) e) times the stress
history of the unscaled run, bit for bit, on the row owner, the fp32 sweep and its 24-bit stream.

Sparse input at N <= 4,097, one launch per case: a case takes a fraction of a second."""
import ctypes
import functools
import os

import numpy
import pytest

from blueberry_amd import _lib
from blueberry_amd.solver import HipEngine, layout_info, weighted_steps
from tests import _pair_model as pm
from tests._pack24_model import uniform_map
from tests._util import bits, cu_count, same_bits
from tests.test_sweep_plan_cpu import plan as sweep_plan

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not pm.HAVE_LONGDOUBLE, reason=pm.LONGDOUBLE_REASON)]

LD = pm.LD
KNOBS = ("BB_ROW_OWNER_MAX", "BB_WAVES_PER_CU", "BB_PAIR", "BB_PACK24", "BB_PACK24_MIN_RUN")
# unit-sweep variants: (layout of _pair_model, environment, copy of _pair_model.COUNTS)
SWEEPS = {
    "f32-wpb8": ("f32", {"BB_WAVES_PER_CU": "8"}, "f32 sweep"),
    "f32-wpb4": ("f32", {"BB_WAVES_PER_CU": "4", "BB_PAIR": "0"}, "f32 sweep"),
    "f64-narrow": ("f64n", {}, "f64 sweep"),
    "f64-wide": ("f64w", {}, "f64 sweep"),
}
WAVES_PER_BLOCK = {"f32-wpb8": 8, "f32-wpb4": 4}
SWEEP_CASES = [(v, e) for v in sorted(SWEEPS) for e in pm.SCALES[pm.LAYOUTS[SWEEPS[v][0]]["dtype"]]]
ROW_OWNER_CASES = [(d, n, e) for d in sorted(pm.ROW_OWNER_SIZES) for n in pm.ROW_OWNER_SIZES[d]
                   for e in pm.SCALES[d]]


def _env(monkeypatch, **env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))


@functools.lru_cache(maxsize=None)
def _case(n, dtype, e, q, layout):
    case = pm.operands(n, dtype, e, q=q, layout=layout)
    case.x.setflags(write=False)
    case.delta.setflags(write=False)
    return case, pm.reference(case, q)


def _sweep_gradient(monkeypatch, case, q, env, want_layout):
    """One grad() on the unit sweep: (g (n_pad, 3), S) as float64 from the exchange buffer."""
    _env(monkeypatch, BB_ROW_OWNER_MAX=0, **env)
    eng = HipEngine(case.n, case.dtype)
    try:
        lay = eng.layout()
        assert (lay["vw"], lay["rows_per_unit"]) == want_layout, lay
        eng.set_wish_sparse(*pm.wish_triples(case), "wish", 1.0)
        eng.set_weight_power(q)
        eng.set_coords(case.x)
        eng.grad()
        eng.sync()
        ex = eng.read_exchange()
        assert eng.iteration_path() == ("units", 0)
        assert numpy.array_equal(eng.degrees(), _degrees(case))     # the map that arrived is the matching
    finally:
        eng.close()
    n_pad = lay["n_pad"]
    assert ex.shape == (3 * n_pad + 2,)
    return ex[:3 * n_pad].reshape(n_pad, 3), float(ex[-2]) + float(ex[-1])


def _degrees(case):
    deg = numpy.ones(case.n, dtype=numpy.int64)
    deg[case.lonely] = 0
    return deg


def _worst(err, unit):
    """max err / unit over the entries with unit > 0; where unit = 0 the error must be 0 too."""
    assert (err[unit == 0] == 0).all()
    k = unit > 0
    return float((err[k] / unit[k]).max())


def _check_gradient(what, g, extra, case, ref, q, copy):
    """Assertion 1 on both ends of every pair (g (n, 3) as longdouble; extra: the read-out's own
    rounding per entry, same shape).  Returns the worst error in units of u * (bound term)."""
    u = pm.U[case.dtype]
    C, _ = pm.bound_factors(copy, q)
    err = numpy.concatenate([numpy.abs(g[case.i] - ref.g) - extra[case.i],
                             numpy.abs(g[case.j] + ref.g) - extra[case.j]])
    unit = numpy.concatenate([ref.unit_g, ref.unit_g]) * u
    err = numpy.maximum(err, 0)
    worst = _worst(err, unit)
    a = int(numpy.argmax(numpy.where(unit > 0, err / numpy.where(unit > 0, unit, 1), 0).max(1))) % case.i.size
    print("PAIR-MATH gradient | %s | q=%d | e=%d | worst %.3f u | count %d | C %d | at %s, delta/d %s"
          % (what, q, case.e, worst, C // 2, C, case.direction[a], case.ratio[a]))
    assert worst <= C, (what, q, case.e, worst, C)
    return worst


def _check_stress(what, S, case, ref, q, copy):
    u = pm.U[case.dtype]
    _, CS = pm.bound_factors(copy, q)
    n = case.i.size
    err = abs(LD(S) - ref.s.sum())
    unit = u * ref.unit_s.sum()
    print("PAIR-MATH stress   | %s | q=%d | e=%d | worst %.3f u | count %d | C_S %d | n %d"
          % (what, q, case.e, float(err / unit), CS // 2, CS, n))
    assert numpy.isfinite(S) and err <= (n + CS) * unit, (what, q, case.e, float(err / unit))


# ---- the unit sweep ----------------------------------------------------------------------------
@pytest.mark.parametrize("q", [0, 1, 2])
@pytest.mark.parametrize("variant,e", SWEEP_CASES)
def test_unit_sweep_pair_by_pair(monkeypatch, variant, e, q):
    layout, env, copy = SWEEPS[variant]
    lay = pm.LAYOUTS[layout]
    n, dtype = pm.SWEEP_SIZES[layout], lay["dtype"]
    case, ref = _case(n, dtype, e, q, layout)
    if variant in WAVES_PER_BLOCK:
        # layout() does not say how many waves a workgroup has: the library's own plan for these
        # knobs on this device does (bb_layout_sweep_plan, what bb_solver_create calls)
        info = layout_info(n, dtype)
        p = sweep_plan(n, _lib.BB_F32, None, 0, info["n_units"], cu_count(),
                       wpc=int(env["BB_WAVES_PER_CU"]), pair=env.get("BB_PAIR", "1") != "0")
        assert p["wpb"] == WAVES_PER_BLOCK[variant], p["wpb"]
    g, S = _sweep_gradient(monkeypatch, case, q, env, (lay["vw"], lay["rows_per_unit"]))
    assert numpy.isfinite(g).all()
    # 2. antisymmetry, no tolerance; 3. the lonely bin and the padding rows: +0.0
    assert numpy.array_equal(g[case.j], -g[case.i])       # finite: equal values are equal bits (zeros: +-0)
    rest = numpy.concatenate([g[case.lonely].ravel(), g[n:].ravel()])
    assert rest.size >= 3 and not bits(rest).any()
    # 1. every component against the longdouble formula; 4. the stress
    _check_gradient(variant, g[:n].astype(LD), numpy.zeros((n, 3), dtype=LD), case, ref, q, copy)
    _check_stress(variant, S, case, ref, q, copy)


# ---- the row owner -----------------------------------------------------------------------------
def _bin_steps(case, ref):
    """A power of two per bin: the move of every component the pair acts on is at least 2^8 times
    the bin's largest coordinate -- from the model's force, or from u times its bound term where
    the model's force is (nearly) nothing, delta = d."""
    u = pm.U[case.dtype]
    force = numpy.where(ref.unit_g > 0, numpy.maximum(numpy.abs(ref.g), u * ref.unit_g), numpy.inf).min(1)
    top = numpy.maximum(numpy.abs(case.x[case.i]).max(1), numpy.abs(case.x[case.j]).max(1)).astype(LD)
    steps = numpy.ones(case.n)
    steps[case.i] = steps[case.j] = 2.0 ** numpy.ceil(numpy.log2((256 * top / force).astype(numpy.float64)))
    return steps


def _row_owner_step(monkeypatch, case, q, steps):
    _env(monkeypatch)
    eng = HipEngine(case.n, case.dtype)
    try:
        eng.set_wish_sparse(*pm.wish_triples(case), "wish", 1.0)
        eng.set_weight_power(q)
        eng.set_bin_steps(steps)
        eng.set_coords(case.x)
        eng.iterate(1, 1.0)
        x1, hist = eng.get_coords(), eng.stress_history()
        assert eng.iteration_path() == ("row_owner", 4 if case.n <= 1024 else 2)
    finally:
        eng.close()
    assert hist.shape == (1,)
    return x1, float(hist[0])


@pytest.mark.parametrize("q", [0, 1, 2])
@pytest.mark.parametrize("dtype,n,e", ROW_OWNER_CASES)
def test_row_owner_pair_by_pair(monkeypatch, dtype, n, e, q):
    T = pm.np_dtype(dtype)
    copy = "f32 row owner" if dtype == "float32" else "f64 row owner"
    what = "%s N=%d" % (copy, n)
    case, ref = _case(n, dtype, e, q, None)
    steps = _bin_steps(case, ref)
    assert (numpy.log2(steps) % 1 == 0).all() and numpy.array_equal(steps.astype(T).astype(numpy.float64), steps)
    x1, S = _row_owner_step(monkeypatch, case, q, steps)
    assert numpy.isfinite(x1).all()
    g = (case.x.astype(LD) - x1.astype(LD)) / steps.astype(LD)[:, None]          # exact
    ulp = numpy.spacing(numpy.abs(x1).astype(T)).astype(LD) / steps.astype(LD)[:, None]
    # 3. the lonely bin stays where it is; the axes' other components do not move either (1.)
    assert same_bits(x1[case.lonely], case.x[case.lonely])
    still = ref.unit_g == 0
    assert still.any() and same_bits(x1[case.i][still], case.x[case.i][still])
    assert same_bits(x1[case.j][still], case.x[case.j][still])
    # 2. the pair is evaluated from both ends: the two moves agree to the rounding of x' alone
    assert (numpy.abs(g[case.i] + g[case.j]) <= (ulp[case.i] + ulp[case.j]) / 2).all()
    _check_gradient(what, g, ulp, case, ref, q, copy)
    _check_stress(what, S, case, ref, q, copy)
    if dtype == "float64":
        # 5. one expression on both paths: x' is x - step * g of the sweep's gradient, bit for bit
        lay = pm.LAYOUTS["f64n"]
        gs, Ss = _sweep_gradient(monkeypatch, case, q, {}, (lay["vw"], lay["rows_per_unit"]))
        assert numpy.array_equal(gs[case.j], -gs[case.i])
        assert same_bits(x1, case.x - steps[:, None] * gs[:n])
        _check_gradient(what + " (sweep)", gs[:n].astype(LD), numpy.zeros((n, 3), dtype=LD), case, ref, q, "f64 sweep")
        _check_stress(what + " (sweep)", Ss, case, ref, q, "f64 sweep")


# ---- the refined fp64 routines themselves ----------------------------------------------------------
PROBE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "probes", "librefined_f64_probe.so")


def _refined_f64(x):
    """(1/sqrt(x), sqrt(x)) of rsqrt_sqrt_f64 and 1/x of rcp_f64 for every x, from the device."""
    assert os.path.exists(PROBE), "%s is missing: build.sh makes it" % PROBE
    _lib.load()                                  # the HIP runtime the library is bound to, first
    fn = ctypes.CDLL(PROBE).bb_probe_refined_f64
    fn.restype = ctypes.c_int
    fn.argtypes = [_lib.p_dbl, _lib.c_i64, _lib.p_dbl, _lib.p_dbl, _lib.p_dbl]
    x = numpy.ascontiguousarray(x, dtype=numpy.float64)
    out = [numpy.full(x.size, numpy.nan) for _ in range(3)]
    rc = fn(_lib.as_f64_ptr(x), x.size, *[_lib.as_f64_ptr(o) for o in out])
    assert rc == 0, "bb_probe_refined_f64: HIP error %d" % rc
    return out


@functools.lru_cache(maxsize=None)
def _refined_operands():
    """Every d^2 and every delta the fp64 cases of this file hold (each operand class, scale and
    weight power), and 4,096 significands spread over [1, 4) at even and odd exponents."""
    xs = []
    for layout in ("f64n", "f64w"):
        for e in pm.SCALES["float64"]:
            case, _ = _case(pm.SWEEP_SIZES[layout], "float64", e, 0, layout)
            dx = case.x[case.i] - case.x[case.j]
            xs += [(dx * dx).sum(1) + 1e-300, case.delta]
    sig = 4.0 ** numpy.random.default_rng(7).random(4096)
    for k in (0, 1, -80, 81, -600, 601):
        xs.append(sig * 2.0 ** k)
    x = numpy.concatenate(xs)
    x.setflags(write=False)
    return x


def test_refined_f64_routines_within_2_ulp():
    """rsqrt_sqrt_f64: "good to the last bit or two"; rcp_f64: the term dropped is e^3 < 2^-78.
    Each result within 2 ulp (of the float64 nearest the true value) of the longdouble one."""
    x = _refined_operands()
    rinv, dist, rcp = _refined_f64(x)
    xl = x.astype(LD)
    worst = {}
    for name, got, want in (("1/sqrt", rinv, 1 / numpy.sqrt(xl)), ("sqrt", dist, numpy.sqrt(xl)), ("1/x", rcp, 1 / xl)):
        assert numpy.isfinite(got).all()
        ulp = numpy.spacing(want.astype(numpy.float64)).astype(LD)
        worst[name] = float((numpy.abs(got.astype(LD) - want) / ulp).max())
    print("PAIR-MATH refined fp64 | %d operands | worst, in ulp: %s"
          % (x.size, ", ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
    assert max(worst.values()) <= 2.0, worst


# ---- scale covariance, bit for bit -----------------------------------------------------------------
def _hic_like(n, dtype, seed=3):
    """A complete Hi-C-like map as wish distances: counts ~ Poisson(200 |i - j|^-1.08) + 1,
    delta = c^(-1/3), rounded to the dtype."""
    rng = numpy.random.default_rng(seed + n)
    i, j = numpy.indices((n, n))
    c = numpy.triu(rng.poisson(200.0 * numpy.maximum(numpy.abs(i - j), 1) ** -1.08) + 1.0, 1)
    w = numpy.where(c > 0, numpy.where(c > 0, c, 1.0) ** (-1.0 / 3.0), 0.0)
    w = (w + w.T).astype(pm.np_dtype(dtype)).astype(numpy.float64)
    return w


def _start(n, w, dtype, seed=1):
    x = numpy.random.default_rng(seed).standard_normal((n, 3)) * float(numpy.median(w[w > 0]))
    return x.astype(pm.np_dtype(dtype)).astype(numpy.float64)


def _fit(n, dtype, w, x0, q, mu, k=5):
    """K steps with lr = 1 / (2 N) (q = 0) or 'auto' from the weighted degrees (q > 0)."""
    eng = HipEngine(n, dtype)
    try:
        eng.set_wish_dense(w, "wish", 1.0)
        lr = 1.0 / (2.0 * n)
        if q:
            eng.set_weight_power(q)
            lr, _ = weighted_steps(eng.weight_sums(), n, dtype, "auto", False)
        eng.set_momentum(mu)
        eng.set_coords(x0)
        eng.iterate(k, lr)
        return eng.get_coords(), eng.stress_history(), eng.iteration_path(), eng.stream_info(), lr
    finally:
        eng.close()


COVARIANCE = {
    # path: (dtype, N, environment, the map)
    "row-owner-f32": ("float32", 513, {}, _hic_like),
    "row-owner-f64": ("float64", 513, {}, _hic_like),
    "sweep-f32": ("float32", 1537, {"BB_ROW_OWNER_MAX": "0", "BB_PACK24": "0"}, _hic_like),
    "sweep-f32-pack24": ("float32", 1537, {"BB_ROW_OWNER_MAX": "0", "BB_PACK24": "1", "BB_PACK24_MIN_RUN": "1"},
                         lambda n, dtype: uniform_map(n)),
}


@pytest.mark.parametrize("q,mu", [(0, 0.0), (0, 0.5), (1, 0.0), (2, 0.0)])
@pytest.mark.parametrize("path", sorted(COVARIANCE))
def test_scale_covariance_bit_for_bit(monkeypatch, path, q, mu):
    """x -> 2^e x, delta -> 2^e delta: the coordinates come out 2^e times, the stress history
    2^((2 - q) e) times, the same significands.  This rests on v_rsq_* / v_rcp_* depending on the
    significand alone under an even shift of the exponent (measured here: docs/MEASUREMENTS.md)."""
    dtype, n, env, make = COVARIANCE[path]
    _env(monkeypatch, **env)
    w = numpy.asarray(make(n, dtype), dtype=numpy.float64)
    x0 = _start(n, w, dtype)
    X, h, route, info, lr = _fit(n, dtype, w, x0, q, mu)
    assert route[0] == ("row_owner" if path.startswith("row-owner") else "units")
    if route[0] == "units":
        assert (info["packed_units"] > 0) == path.endswith("pack24")
    assert h.shape == (5,) and numpy.isfinite(h).all() and (h > 0).all() and numpy.isfinite(X).all()
    for e in ((-20, 20) if dtype == "float32" else (-200, 200)):
        f = 2.0 ** e
        Xe, he, route_e, info_e, lr_e = _fit(n, dtype, w * f, x0 * f, q, mu)
        assert route_e == route and info_e["packed_units"] == info["packed_units"]
        assert lr_e == lr * 2.0 ** (q * e)
        same_x, same_h = same_bits(Xe, X * f), same_bits(he, h * 2.0 ** ((2 - q) * e))
        print("PAIR-MATH covariance | %s | q=%d | mu=%.1f | e=%d | coordinates %s | history %s"
              % (path, q, mu, e, "same bits" if same_x else "DIFFER", "same bits" if same_h else "DIFFER"))
        assert same_x and same_h, (path, q, mu, e)
