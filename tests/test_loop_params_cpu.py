"""CPU guards of tests/test_gpu_loop_params.py, on the same case table (tests/loop_param_cases.py): no device needed.

  discriminating power  a kernel that ignored BOTH α and σ must fail the GPU test: the oracle's x at the tested (α, σ) differs from its x at the
                        defaults by at least 1000 x the fp64 bound the GPU test applies (10 x the fp32 bound where the case runs in fp32), in every
                        column.  One that ignored σ ALONE fails the fp64 runs (σ alone moves x by 1000 x the fp64 bound, asserted) but not the
                        fp32 ones: there σ alone moves x by less than the 2e-3 bound, and the fp64 instantiation of the same template stands in.
  stall stop            on the inconsistent-equality cases the oracle ends by convAdmm, with margin on both sides in the step |x - xp|, and a
                        max for the min of ϵAdmm (:34) would end at another check: the oracle with both tolerances at the larger value does.
  no knife edge         every run that asserts the oracle's stopping iteration has margin on both sides of the stop: at the stopping check both
                        residuals lie at or below 0.999 of their thresholds, at the check one period earlier one lies at or above 1.001 of its
                        threshold.  GPU and oracle agree to about 1e-9, six orders below that margin.  The two tolerance orders must also stop at
                        different checks somewhere in the case, or a kernel that swapped ϵAbs and ϵRel would pass.
  second oracle         qps_oracle_np.SolveQuadraticProgramRefLoop (a separate restatement of the reference loop) agrees with the C oracle at
                        the non-default (α, σ) to 1e-12, and gives the same flag, iteration and NaN proposal on the exact fixed point."""
import math

import numpy as np
import pytest

import loop_param_cases as C

IDS = [i.key for i in C.IMPLS]


def _thresholds(io, params):
    ea, er = params["epsAbs"], params["epsRel"]
    return ea + er * io["maxNormPrim"], ea + er * io["maxNormDual"]                  # SolveQuadraticProgram.jl:99-100


def _assert_margin(c_oracle, impl, col, params, where, to_tolerance=False):
    """The oracle stops by convPrimDual, with margin at that check and at the one before.  Returns its stopping iteration."""
    _, io = C.oracle_run(c_oracle, impl, col, to_tolerance, **params)
    period = params.get("numItrConv", impl.kw.get("numItrConv", 25))
    assert io["convFlag"] == 3 and period < io["iterations"] < params["numIterations"], (where, io["convFlag"], io["iterations"])
    tp, td = _thresholds(io, params)
    assert io["resPrim"] <= 0.999 * tp and io["resDual"] <= 0.999 * td, (where, io["resPrim"] / tp, io["resDual"] / td)
    cut = dict(params, numIterations=io["iterations"] - period)
    _, ic = C.oracle_run(c_oracle, impl, col, to_tolerance, **cut)
    tp, td = _thresholds(ic, cut)
    assert ic["convFlag"] == 1 and ic["iterations"] == io["iterations"] - period
    assert ic["resPrim"] >= 1.001 * tp or ic["resDual"] >= 1.001 * td, (where, ic["resPrim"] / tp, ic["resDual"] / td)
    return io["iterations"]


@pytest.mark.parametrize("impl", C.IMPLS, ids=IDS)
def test_fixed_k_cases_tell_the_tested_scalars_from_the_defaults(c_oracle, impl):
    assert 10 <= impl.K <= 60
    dtypes = ("f64", "f32") if impl.key in C.FP32_FIXED_K else ("f64",)
    need = max([1000 * C.TOL["f64"]["x"]] + [10 * C.TOL[d]["x"] for d in dtypes if d == "f32"])
    for b, col in enumerate(C.columns(impl)):                                        # (the fp32 runs of a case use the same shape and data)
        assert all(C.shape_of(impl, d) == impl.shape for d in dtypes)
        x_def, _ = C.oracle_run(c_oracle, impl, col, **C.fixed_k(impl, *C.DEFAULT))
        for alpha, sigma in C.PARAM_SEQUENCE[1:-1]:
            x, _ = C.oracle_run(c_oracle, impl, col, **C.fixed_k(impl, alpha, sigma))
            assert C.rel(x, x_def) >= need, (impl.key, b, alpha, sigma, C.rel(x, x_def), need)
            if sigma != C.DEFAULT[1]:                                                # σ alone, at the tested α
                x_s, _ = C.oracle_run(c_oracle, impl, col, **C.fixed_k(impl, alpha, C.DEFAULT[1]))
                assert C.rel(x, x_s) >= 1000 * C.TOL["f64"]["x"], (impl.key, b, alpha, sigma, C.rel(x, x_s))


@pytest.mark.parametrize("impl", C.IMPLS, ids=IDS)
def test_split_tolerance_cases_stop_with_margin(c_oracle, impl):
    stops = {}
    for tag, params in C.split_runs(impl):
        stops[tag] = [_assert_margin(c_oracle, impl, col, params, (impl.key, tag, b), True)
                      for b, col in enumerate(C.columns(impl, to_tolerance=True))]
    fixed = [stops[t] for t, _ in C.split_runs(impl)[:2]]
    assert any(a != b for a, b in zip(*fixed)), (impl.key, fixed)                    # swapping ϵAbs and ϵRel changes the stopping iteration
    assert max(max(v) for v in fixed) <= 1500                                        # about a thousand iterations at most: the GPU runs stay short


def test_adaptive_cases_tell_the_tested_factor_from_the_default(c_oracle):
    """With fctrΡ = 2 and numItrConv = 7 the (64, 128) run refactors 3 times and the (200, 330) run twice; at the default fctrΡ = 5 both refactor
    once -- so a loop that ignored fctrΡ cannot reproduce the oracle's numRefactor.  (The issue quotes 4 refactors for (64, 128); that figure was
    not reproduced with these parameters, the oracle gives 3.)"""
    for key, want in (("reg", 3), ("fused_graph", 2)):
        impl = C.BY_KEY[key]
        col = C.columns(impl, to_tolerance=True)[0]
        params = dict(C.split_runs(impl)[2][1])
        _, io = C.oracle_run(c_oracle, impl, col, **params)
        _, i5 = C.oracle_run(c_oracle, impl, col, **dict(params, fctrRho=5.0))
        assert (io["numRefactor"], i5["numRefactor"]) == (want, 1), (key, io["numRefactor"], i5["numRefactor"])


def test_the_oracle_plugins_agree_within_the_bounds_on_the_cg_cases(c_oracle):
    """The reference's CG plugins stop their inner solve at max(sqrt(eps) ||r0||, ϵPcg), so its own plugins differ from one another by roundoff
    amplified through that rule.  The GPU tests hold the CG routes to the fp64 bounds of the Cholesky route, which only means something on
    a case where the oracle's matrix-free CG, explicit CG and Cholesky agree within those bounds themselves (fixed K), and where its CG and
    L D L' plugins agree on rhoFinal well below the 1e-9 the adaptive run is held to."""
    impl, tol = C.BY_KEY["cg_explicit"], C.TOL["f64"]
    P, q, A, l, u, x0 = C.columns(impl)[0]
    for alpha, sigma in C.PARAM_SEQUENCE[:-1]:
        params = C.fixed_k(impl, alpha, sigma)
        runs = [c_oracle.solve(P, q, A, l, u, **params, **C.oracle_kw(C.BY_KEY[k])) for k in ("cg_matfree", "cg_explicit")]
        runs.append(c_oracle.solve(P.toarray(), q, A.toarray(), l, u, **params))
        for i in range(3):
            for j in range(i + 1, 3):
                (xa, ia), (xb, ib) = runs[i], runs[j]
                assert C.rel(xa, xb) <= tol["x"] and C.rel(ia["z"], ib["z"]) <= tol["z"] and C.rel(ia["y"], ib["y"]) <= tol["y"], (alpha, sigma, i, j)
                for k in ("resPrim", "resDual"):
                    assert abs(ia[k] - ib[k]) <= tol[k] * max(1.0, ib[k]), (alpha, sigma, i, j, k)
    col = C.columns(impl, to_tolerance=True)[0]
    params = C.split_runs(impl)[2][1]
    _, icg = C.oracle_run(c_oracle, impl, col, True, **params)
    _, ild = C.oracle_run(c_oracle, C.BY_KEY["ldl"], col, **params)
    assert icg["numRefactor"] == ild["numRefactor"] == 1 and icg["iterations"] == ild["iterations"]
    assert abs(icg["rhoFinal"] / ild["rhoFinal"] - 1.0) <= 5e-10


def _step(c_oracle, impl, col, it):
    """max(|x - xp|, |z - zp|) of iteration ``it``: what :105 compares with ϵAdmm (from two runs of the oracle with ϵ = 0)."""
    kw = dict(C.STALL, epsAbs=0.0, epsRel=0.0)
    xa, ia = C.oracle_run(c_oracle, impl, col, **dict(kw, numIterations=it))
    xb, ib = C.oracle_run(c_oracle, impl, col, **dict(kw, numIterations=it - 1))
    return max(np.abs(xa - xb).max(), np.abs(ia["z"] - ib["z"]).max())


@pytest.mark.parametrize("impl", C.IMPLS, ids=IDS)
def test_stall_cases_stop_with_margin_and_tell_min_from_max(c_oracle, impl):
    eps_admm = min(C.STALL["epsAbs"], C.STALL["epsRel"]) * 1e-2
    larger = max(C.STALL["epsAbs"], C.STALL["epsRel"])
    period = impl.kw.get("numItrConv", 25)
    for b, col in enumerate(C.stall_columns(impl)):
        _, io = C.oracle_run(c_oracle, impl, col, **C.STALL)
        assert io["convFlag"] == 2 and 2 * period <= io["iterations"] < C.STALL["numIterations"], (impl.key, b, io["convFlag"], io["iterations"])
        assert io["resPrim"] > 10 * (C.STALL["epsAbs"] + C.STALL["epsRel"] * io["maxNormPrim"])      # convPrimDual is nowhere near
        assert _step(c_oracle, impl, col, io["iterations"]) <= 0.999 * eps_admm, (impl.key, b)
        assert _step(c_oracle, impl, col, io["iterations"] - period) >= 1.001 * eps_admm, (impl.key, b)
        _, im = C.oracle_run(c_oracle, impl, col, **dict(C.STALL, epsAbs=larger, epsRel=larger))     # ϵAdmm as a max for the min would give it
        assert im["convFlag"] == 2 and im["iterations"] < io["iterations"], (impl.key, b, im["iterations"], io["iterations"])


@pytest.mark.parametrize("key", C.GRAPH_ROUTES)
def test_check_period_cases_stop_with_margin_before_the_last_check(c_oracle, key):
    impl = C.BY_KEY[key]
    col = C.columns(impl)[0]
    for tag, params in C.period_runs(impl):
        nc = params["numItrConv"]
        if params["epsAbs"] == 0.0:
            _, io = C.oracle_run(c_oracle, impl, col, **params)
            assert io["convFlag"] == 1 and io["iterations"] == C.PERIOD_ITERATIONS and C.PERIOD_ITERATIONS % nc != 0
            continue
        it = _assert_margin(c_oracle, impl, col, params, (key, tag))
        assert it < (C.PERIOD_ITERATIONS // nc) * nc, (key, tag, it)


@pytest.mark.parametrize("impl", [i for i in C.IMPLS if i.kind != "csc"], ids=lambda i: i.key)
def test_second_oracle_agrees_off_the_defaults(c_oracle, np_oracle, impl):
    for col in C.columns(impl):
        P, q, A, l, u, x0 = col
        for alpha, sigma in C.PARAM_SEQUENCE[1:-1]:
            xc, ic = C.oracle_run(c_oracle, impl, col, **C.fixed_k(impl, alpha, sigma))
            xn = x0.copy(); info = {}
            np_oracle.SolveQuadraticProgramRefLoop(xn, P, q, A, l, u, np_oracle.RedCholInit, np_oracle.RedChol, numIterations=impl.K, ϵAbs=0.0, ϵRel=0.0,
                                                   ρ=C.RHO, σ=sigma, α=alpha, numItrConv=impl.kw.get("numItrConv", 25), info=info)
            assert C.rel(xn, xc) <= 1e-12 and C.rel(info["z"], ic["z"]) <= 1e-12 and C.rel(info["y"], ic["y"]) <= 1e-12, (impl.key, alpha, sigma)


@pytest.mark.parametrize("eps", [0.0, 1e-6])
@pytest.mark.parametrize("period", [25, 7])
def test_both_oracles_on_the_exact_fixed_point(c_oracle, np_oracle, period, eps):
    """0 <= ϵAdmm holds while 0 < 0 does not, and :105-107 overrides :102-104: convAdmm at the first check for ϵ = 0 and for ϵ = 1e-6.  The
    proposed ρ is 0 / 0."""
    impl = C.BY_KEY["reg"]
    P, q, A, l, u, x0 = C.trivial(C.columns(impl)[0])
    for adpt in (False, True):
        xc, ic = C.oracle_run(c_oracle, impl, (P, q, A, l, u, x0), numIterations=200, numItrConv=period, epsAbs=eps, epsRel=eps, rho=C.RHO, adptRho=adpt)
        xn = x0.copy(); info = {}
        flag = np_oracle.SolveQuadraticProgramRefLoop(xn, P, q, A, l, u, np_oracle.RedCholInit, np_oracle.RedChol, numIterations=200, numItrConv=period,
                                                      ϵAbs=eps, ϵRel=eps, ρ=C.RHO, adptΡ=adpt, info=info)
        assert ic["convFlag"] == int(flag) == 2 and ic["iterations"] == info["iterations"] == period
        assert ic["numRefactor"] == info["n_refactor"] == 0
        assert not xc.any() and not xn.any() and not ic["z"].any() and not ic["y"].any() and ic["resPrim"] == ic["resDual"] == 0.0
        if adpt:
            assert math.isnan(ic["rhoProposed"]) and math.isnan(info["rho_proposed"])
        else:
            assert ic["rhoProposed"] == info["rho_proposed"] == C.RHO


@pytest.mark.parametrize("impl", C.IMPLS, ids=IDS)
def test_every_keyword_of_the_table_is_one_of_the_solve_signature(impl):
    """The GPU tests pass the table's scalars through **: a misspelled keyword must show here, not on the device."""
    import inspect
    from quadraticprogramsolver_amd import solver
    fn = {"batch": solver.QuadraticProgramBatch.solve, "shared": solver.QuadraticProgramSharedBatch.solve}.get(impl.kind, solver.QuadraticProgram.solve)
    names = set(inspect.signature(fn).parameters)
    runs = [C.fixed_k(impl, *C.DEFAULT), C.STALL] + [p for _, p in C.split_runs(impl)] + ([p for _, p in C.period_runs(impl)] if impl.key in C.GRAPH_ROUTES else [])
    for dtype in ("f64", "f32"):
        for params in runs:
            assert set(C.solver_kw(impl, dtype)) | set(C.api_kw(params)) <= names, (impl.key, sorted((set(C.solver_kw(impl, dtype)) | set(C.api_kw(params))) - names))
