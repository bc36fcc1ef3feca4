"""Every implementation of the ADMM row update (SolveQuadraticProgram.jl:56-61) and of the stopping decision (:79-112) off the defaults of the
reference signature: α and σ away from 1.6 and 1e-6, ϵAbs != ϵRel, odd and even check periods, fctrΡ = 2, and the exact fixed point on which `<=`
and `<` and the order of the two convergence tests decide the flag.  The cases, the route each one takes and how that was confirmed are in
tests/loop_param_cases.py; tests/test_loop_params_cpu.py checks on the CPU that every case would fail a kernel that ignored the scalar under test
and that no case asserting a stopping iteration sits on a knife edge.  Every comparison is with c_oracle.solve called with the same parameters.

Measured on an MI355X (every figure is printed before its assertion; run with -s).  Fixed K, fp64, bounds 1e-9 (x, z, residuals) and 1e-8 (y): the
dense routes, the three batch forms and L D L' stay within 9e-15 on x / z / y and 5e-14 on the residuals; the CG routes within 1.5e-11 on x / z / y
and 9.4e-11 on the residuals, a margin of 10 (their inner solve stops at max(sqrt(eps) ||r0||, ϵPcg) as the reference's does, and the oracle's own
plugins differ by 5.5e-10 on that case).  fp32 register kernel: 3.2e-7 / 1.7e-6 / 2.3e-7 on x / z / y against 2e-3 / 2e-3 / 2e-2, residuals 4.7e-6.  To a tolerance,
fp64: flags, stopping iterations and refactor counts equal on every route and column, max|x - x_oracle| <= 6e-14 against 1e-5, residuals within
2.1e-13 against 1e-9, rhoFinal within the asserted 1e-9 relative (printed to six digits only); the stall runs (275 to 4925 iterations) within
1.9e-13 on x and 2.3e-12 on the residuals.  fp32 to a tolerance: the oracle's flag and iteration count, x within 3.4e-7."""
import contextlib
import math

import numpy as np
import pytest

import loop_param_cases as C
from test_gpu_parity import ABS_DEV_THR, rel

pytestmark = pytest.mark.gpu
IDS = [i.key for i in C.IMPLS]


@contextlib.contextmanager
def handle(gpu, impl, dtype, cols):
    if impl.kind == "batch":
        h = gpu.QuadraticProgramBatch([c[:5] for c in cols], dtype=dtype)
    elif impl.kind == "shared":
        h = gpu.QuadraticProgramSharedBatch(cols[0][0], cols[0][2], np.stack([c[1] for c in cols]), np.stack([c[3] for c in cols]),
                                            np.stack([c[4] for c in cols]), dtype=dtype)
    else:
        P, q, A, l, u, _ = cols[0]
        h = gpu.QuadraticProgram(P, q, A, l, u, dtype=dtype, **({"linsys": impl.linsys} if impl.kind == "csc" else {}))
    try:
        yield h
    finally:
        h.close()


def solve(h, impl, dtype, cols, params, reuseFactor=False):
    """One solve on the case's handle; per column (x, z, y, info).  ``params`` in the oracle's spelling."""
    kw = C.solver_kw(impl, dtype)
    kw.update(C.api_kw(params))
    if impl.kind in ("batch", "shared"):
        X, flags, infos = h.solve(np.stack([c[5] for c in cols]), reuseFactor=reuseFactor, **kw)
        Z, Y = h.dual()
        assert [int(f) for f in flags] == [i["convFlag"] for i in infos]
        return [(X[b], Z[b], Y[b], infos[b]) for b in range(len(cols))]
    x = cols[0][5].copy(); info = {}
    flag = h.solve(x, info=info, reuseFactor=reuseFactor, **kw)
    z, y = h.dual()
    assert int(flag) == info["convFlag"]
    if impl.kind == "dense":
        assert (info["sweepVariant"] == 4) == (impl.small and kw.get("loopVariant", 0) == 0), (impl.key, info["sweepVariant"])   # single launch or not
    else:
        assert info["cgExplicit"] == (1 if impl.linsys == "cg_explicit" else 0), (impl.key, info)
    return [(x, z, y, info)]


def set_env(monkeypatch, impl):
    for k, v in impl.env.items():
        monkeypatch.setenv(k, v)


_oracle = {}


def oracle(c_oracle, impl, cols, tag, params, to_tolerance=False):
    """The oracle's run of every column, computed once per case and shared by the tests that need it."""
    key = (impl.key, cols[0][0].shape, cols[0][2].shape, tag)
    if key not in _oracle:
        _oracle[key] = [C.oracle_run(c_oracle, impl, col, to_tolerance, **params) for col in cols]
    return _oracle[key]


def assert_iterates(impl, dtype, got, ref, params, what):
    tol = C.TOL[dtype]
    assert params["numIterations"] >= params.get("numItrConv", impl.kw.get("numItrConv", 25))      # a check ran: there are residuals to compare
    for b, ((x, z, y, info), (xo, io)) in enumerate(zip(got, ref)):
        fig = dict(x=rel(x, xo), z=rel(z, io["z"]), y=rel(y, io["y"]), resPrim=abs(info["resPrim"] - io["resPrim"]) / max(1.0, io["resPrim"]),
                   resDual=abs(info["resDual"] - io["resDual"]) / max(1.0, io["resDual"]))
        print(f"{impl.key} {dtype} {what} column {b}: " + " ".join(f"{k} {v:.2e}" for k, v in fig.items()))
        assert info["iterations"] == io["iterations"] and info["convFlag"] == io["convFlag"], (impl.key, what, b, info, io["iterations"])
        for k, v in fig.items():
            assert v <= tol[k], (impl.key, dtype, what, b, k, v)


def assert_to_tolerance(impl, got, ref, what):
    for b, ((x, z, y, info), (xo, io)) in enumerate(zip(got, ref)):
        dev = np.abs(x - xo).max()
        print(f"{impl.key} {what} column {b}: flag {info['convFlag']}/{io['convFlag']} iterations {info['iterations']}/{io['iterations']} "
              f"numRefactor {info['numRefactor']}/{io['numRefactor']} rhoFinal {info['rhoFinal']:.6g}/{io['rhoFinal']:.6g} max|x - x_oracle| {dev:.2e} "
              f"|dresPrim| {abs(info['resPrim'] - io['resPrim']):.2e} |dresDual| {abs(info['resDual'] - io['resDual']):.2e}")
        assert info["convFlag"] == io["convFlag"] and info["iterations"] == io["iterations"], (impl.key, what, b)
        assert info["numRefactor"] == io["numRefactor"] and info["rhoFinal"] == pytest.approx(io["rhoFinal"], rel=1e-9), (impl.key, what, b)
        assert abs(info["resPrim"] - io["resPrim"]) <= 1e-9 * max(1.0, io["resPrim"]), (impl.key, what, b)
        assert abs(info["resDual"] - io["resDual"]) <= 1e-9 * max(1.0, io["resDual"]), (impl.key, what, b)
        assert dev <= ABS_DEV_THR, (impl.key, what, b, dev)


FIXED_K = [(i, "f64") for i in C.IMPLS] + [(C.BY_KEY[k], "f32") for k in C.FP32_FIXED_K]


@pytest.mark.parametrize("reuse", [False, True], ids=["fresh_factor", "reuseFactor"])
@pytest.mark.parametrize("impl,dtype", FIXED_K, ids=[f"{i.key}-{d}" for i, d in FIXED_K])
def test_fixed_k_iterates_off_the_default_alpha_and_sigma(gpu, c_oracle, monkeypatch, impl, dtype, reuse):
    """ϵ = 0, ρ = 0.1, K iterations with a check every 10 (so the last iteration reports residuals) on ONE handle: defaults, (α, σ) = (1.0, 1e-6), (1.9, 1e-2), (0.5, 1.0), defaults again -- each against the oracle
    at the same scalars, every column, batch warm starts non-zero.  The last run repeats the first bit for bit: a graph replayed with another α or
    a factor kept across a change of σ would not."""
    set_env(monkeypatch, impl)
    cols = C.columns(impl, dtype)
    runs = []
    with handle(gpu, impl, dtype, cols) as h:
        for alpha, sigma in C.PARAM_SEQUENCE:
            params = C.fixed_k(impl, alpha, sigma)
            got = solve(h, impl, dtype, cols, params, reuseFactor=reuse)
            assert_iterates(impl, dtype, got, oracle(c_oracle, impl, cols, ("fixed_k", alpha, sigma), params), params, f"alpha={alpha} sigma={sigma}")
            runs.append(got)
    for (x0, z0, y0, i0), (x1, z1, y1, i1) in zip(runs[0], runs[-1]):
        assert np.array_equal(x0, x1) and np.array_equal(z0, z1) and np.array_equal(y0, y1)
        assert (i0["resPrim"], i0["resDual"]) == (i1["resPrim"], i1["resDual"])


@pytest.mark.parametrize("key", C.GRAPH_ROUTES)
def test_check_periods_and_graph_run_lengths(gpu, c_oracle, key):
    """numIterations = 37 with numItrConv = 3, 4 and 7 where plain iterations are replayed from a graph: even runs cut out of odd and even periods,
    and a tail shorter than a period.  To ϵ = 0 (37 iterations) and to a tolerance at which the oracle stops at a check that is not the last:
    same flag, same iteration count, same iterates."""
    impl = C.BY_KEY[key]
    cols = C.columns(impl)
    with handle(gpu, impl, "f64", cols) as h:
        for tag, params in C.period_runs(impl):
            got = solve(h, impl, "f64", cols, params)
            assert_iterates(impl, "f64", got, oracle(c_oracle, impl, cols, tag, params), params, tag)


@pytest.mark.parametrize("impl", C.IMPLS, ids=IDS)
def test_split_tolerances(gpu, c_oracle, monkeypatch, impl):
    """(ϵAbs, ϵRel) = (1e-3, 1e-9) and (1e-9, 1e-3) at ρ = 0.1, and (1e-3, 1e-9) with adptΡ, fctrΡ = 2, numItrConv = 7 where the route adapts ρ:
    flag, stopping iteration, numRefactor, rhoFinal and residuals of the oracle.  The two orders stop at different checks, so swapped tolerances
    or an ignored fctrΡ cannot pass (margins: tests/test_loop_params_cpu.py).  These runs end by convPrimDual long before the step reaches even
    1e-2 of the larger tolerance: they do NOT tell min from max in ϵAdmm, test_stall_stop_takes_the_smaller_tolerance does."""
    set_env(monkeypatch, impl)
    cols = C.columns(impl, to_tolerance=True)
    with handle(gpu, impl, "f64", cols) as h:
        for tag, params in C.split_runs(impl):
            got = solve(h, impl, "f64", cols, params)
            assert_to_tolerance(impl, got, oracle(c_oracle, impl, cols, tag, params, True), tag)


@pytest.mark.parametrize("impl", C.IMPLS, ids=IDS)
def test_stall_stop_takes_the_smaller_tolerance(gpu, c_oracle, monkeypatch, impl):
    """ϵAdmm = min(ϵAbs, ϵRel) * 1e-2 (:34) with (ϵAbs, ϵRel) = (1e-2, 1e-4) on inconsistent equality rows: the residuals stay O(1), so the run ends by
    convAdmm when the step falls to 1e-6 -- flag, stopping iteration, x and residuals of the oracle, every column.  A max for the min stops at a
    step of 1e-4, hundreds of iterations earlier (tests/test_loop_params_cpu.py asserts that and the margins)."""
    set_env(monkeypatch, impl)
    cols = C.stall_columns(impl)
    with handle(gpu, impl, "f64", cols) as h:
        got = solve(h, impl, "f64", cols, C.STALL)
        ref = oracle(c_oracle, impl, cols, "stall", C.STALL)
        assert all(io["convFlag"] == 2 for _, io in ref)
        assert_to_tolerance(impl, got, ref, "stall")


@pytest.mark.parametrize("key", C.FP32_FIXED_K)
def test_split_tolerances_fp32(gpu, c_oracle, key):
    """The bounds of test_fp32_path: a convergence flag and x within 1e-3 relative (no iteration equality is claimed for fp32)."""
    impl = C.BY_KEY[key]
    cols = C.columns(impl, "f32", to_tolerance=True)
    with handle(gpu, impl, "f32", cols) as h:
        for tag, params in C.split_runs(impl):
            (x, _, _, info), = solve(h, impl, "f32", cols, params)
            (xo, io), = oracle(c_oracle, impl, cols, tag, params, True)
            print(f"{key} f32 {tag}: flag {info['convFlag']}/{io['convFlag']} iterations {info['iterations']}/{io['iterations']} rel x {rel(x, xo):.2e}")
            assert info["convFlag"] in (2, 3) and np.abs(x - xo).max() <= 1e-3 * max(1.0, np.abs(xo).max())


def _assert_fixed_point(impl, res, period, adpt, what):
    x, z, y, info = res
    assert info["convFlag"] == 2 and info["iterations"] == period, (impl.key, what, info)      # convAdmm at the first check (:105-107 after :102-104)
    assert not x.any() and not z.any() and not y.any(), (impl.key, what)
    assert info["resPrim"] == 0.0 and info["resDual"] == 0.0 and info["numRefactor"] == 0, (impl.key, what, info)
    if adpt:
        assert math.isnan(info["rhoProposed"]), (impl.key, what, info["rhoProposed"])            # 0 / 0, and clamp keeps a NaN


@pytest.mark.parametrize("period", [25, 7])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("impl", C.IMPLS, ids=IDS)
def test_exact_fixed_point(gpu, monkeypatch, impl, dtype, period):
    """q = 0, l = -1, u = 1, x0 = 0 on the case's P and A: every iterate is exactly zero in any arithmetic, so the reference stops with convAdmm at
    iteration numItrConv for ϵ = 0 (0 <= ϵAdmm holds, 0 < 0 does not) and for ϵ = 1e-6 (both tests hold, :105-107 overrides :102-104); with adptΡ
    the proposal is 0 / 0 = NaN and nothing is refactored.  Both oracles give exactly that (tests/test_loop_params_cpu.py).
    fused_eager runs with its own numItrConv = 2 (a longer period would replay graphs).  In the batches ONE column is the trivial one: it stops at the first check while the others run on, and theirs are bit-identical to the same
    batch with an ordinary QP in that place."""
    set_env(monkeypatch, impl)
    period = impl.kw.get("numItrConv", period)                                                      # fused_eager stays eager: a check every 2
    cols = C.columns(impl, dtype)
    modes = [(eps, adpt) for eps in (0.0, 1e-6) for adpt in ((False, True) if impl.adpt else (False,))]
    if impl.kind in ("dense", "csc"):
        fp = [C.trivial(cols[0])]
        with handle(gpu, impl, dtype, fp) as h:
            for eps, adpt in modes:
                params = dict(numIterations=200, numItrConv=period, epsAbs=eps, epsRel=eps, rho=C.RHO, adptRho=adpt)
                _assert_fixed_point(impl, solve(h, impl, dtype, fp, params)[0], period, adpt, (dtype, eps, adpt))
        return
    t = 2                                                                                           # (column 1 of the shared family keeps its l = -Inf rows)
    mixed = list(cols); mixed[t] = C.trivial(cols[t])
    out = {}
    for name, cc in (("mixed", mixed), ("ordinary", cols)):
        with handle(gpu, impl, dtype, cc) as h:
            for eps, adpt in modes:
                params = dict(numIterations=60, numItrConv=period, epsAbs=eps, epsRel=eps, rho=C.RHO, adptRho=adpt)
                out[name, eps, adpt] = solve(h, impl, dtype, cc, params)
    for eps, adpt in modes:
        got, plain = out["mixed", eps, adpt], out["ordinary", eps, adpt]
        _assert_fixed_point(impl, got[t], period, adpt, (dtype, eps, adpt))
        for b in range(len(cols)):
            if b == t:
                continue
            (x, z, y, info), (xp, zp, yp, ip) = got[b], plain[b]
            assert info["iterations"] > period, (impl.key, b, info)                                 # the others run on ...
            assert (info["convFlag"], info["iterations"], info["numRefactor"]) == (ip["convFlag"], ip["iterations"], ip["numRefactor"]), (impl.key, b)
            assert np.array_equal(x, xp) and np.array_equal(z, zp) and np.array_equal(y, yp), (impl.key, dtype, eps, adpt, b)   # ... unchanged
