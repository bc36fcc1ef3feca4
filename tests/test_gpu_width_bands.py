"""The fused pass and the fused sweep of the dense loop in every width band, both types: K = 20 iterations with a check every 10 (so the plain AND the
CHECK instantiation of the pass run and the last iteration reports residuals) at ϵ = 0, ρ = 0.1 and a non-zero warm start, against the structured
fp64 reference of tests/width_band_cases.py -- which also holds the case table, the instantiation every case reaches and the dispatch line that sends
it there, the bounds, and the figures measured on an MI355X.  tests/test_width_bands_cpu.py checks on the CPU that the reference equals the project's
oracles and that every case would fail a kernel that mishandled its top chunk.  Every figure is printed before its assertion (run with -s)."""
import time

import pytest

import loop_param_cases as C
import width_band_cases as W

pytestmark = pytest.mark.gpu


def _report(tag, case, fig, bound, t0):
    print(f"{tag} {W.case_id(case)}: " + " ".join(f"{k} {v:.2e}/{bound[k]:.1e}" for k, v in fig.items()) + f" wall {time.perf_counter() - t0:.1f} s")


def _admm(h, case, f, ref, bound, t0, tag, **extra):
    params = dict(numIterations=W.K, numItrConv=W.PERIOD, epsAbs=0.0, epsRel=0.0, rho=W.RHO, sigma=W.SIGMA, alpha=W.ALPHA, **extra)
    x, info = f.x0.copy(), {}
    h.solve(x, info=info, **C.api_kw(params))
    z, y = h.dual()
    fig = W.errors(dict(x=x, z=z, y=y, resPrim=info["resPrim"], resDual=info["resDual"]), ref, W.ADMM_KEYS)
    _report(tag, case, fig, bound, t0)
    assert info["iterations"] == W.K and info["convFlag"] == 1, info
    assert info["sweepVariant"] == W.sweep_variant(case.dtype, case.NP) == 2 and info["trsvBlock"] == case.nb, (info["sweepVariant"], info["trsvBlock"])
    for k, v in fig.items():
        assert v <= bound[k], (W.case_id(case), tag, k, v, bound[k])
    return info


@pytest.mark.parametrize("case", W.CASES, ids=W.case_id)
def test_admm_iterates_match_the_structured_reference(gpu, case):
    t0 = time.perf_counter()
    f = W.family(case)
    ref, bound = W.admm_loop(W.Structured(f)), W.bounds(case)
    h = gpu.QuadraticProgram(f.dense_P(), f.q, f.A, f.l, f.u, dtype=case.dtype)
    try:
        _admm(h, case, f, ref, bound, t0, "admm")
        if case.dtype == "f64" and case.n == W.ADAPTIVE_N:             # the proposal of the first check crosses fctrΡ: iterations 11 to 20 on a new factor
            ra = W.admm_loop(W.Structured(f), adpt=True, fctr=W.ADMM_FCTR)
            info = _admm(h, case, f, ra, bound, t0, "admm adaptive", adptRho=True, fctrRho=W.ADMM_FCTR)
            assert info["numRefactor"] == ra["numRefactor"] == 1 and info["rhoFinal"] == pytest.approx(ra["rhoFinal"], rel=1e-9)
            assert info["rhoProposed"] == pytest.approx(ra["rhoProposed"], rel=1e-9)
    finally:
        h.close()


def _proxqp(gpu, case, f, P, ref, bound, t0, tag, adpt=False, variant=0):
    me = f.me
    with gpu.ProxQP(P, f.q, f.A[:me], f.b, f.A[me:], f.dd, f.x0, f.y0, f.z0, f.s0, dtype=case.dtype) as prob:   # explicit state (ProxQP.jl:36): isolates the loop
        rg = gpu.SolveQuadraticProgramProxQP(prob, numIterations=W.K, numItrConv=W.PERIOD, ϵAbs=0.0, ϵRel=0.0, ρ=W.PQ_RHO, σ=W.PQ_SIGMA, adptΡ=adpt,
                                             τ=W.PQ_TAU, loopVariant=variant)
        got = dict(x=prob.vX, y=prob.vY, z=prob.vZ, s=prob.vS, resPrim=rg["PrimalResidual"], resDual=rg["DualResidual"])
    fig = W.errors(got, ref, W.PQ_KEYS)
    _report(tag, case, fig, bound, t0)
    assert not rg["Converged"] and rg["Iterations"] == W.K and rg["σ"] == W.PQ_SIGMA, rg
    assert rg["ρ"] == pytest.approx(ref["rho"], rel=1e-9 if case.dtype == "f64" else 1e-3), (rg["ρ"], ref["rho"])
    for k, v in fig.items():
        assert v <= bound[k], (W.case_id(case), tag, k, v, bound[k])


@pytest.mark.parametrize("case", W.PQ_CASES, ids=W.case_id)
def test_proxqp_state_and_report_match_the_structured_reference(gpu, case):
    """G = [A; C] with 701 equality and 1429 inequality rows through the MODE 1 pass (loopVariant 0); one fp64 case also runs the unfused loop
    (loopVariant 1) and one the adaptive ρ, each from a fresh handle seeded with the same explicit state."""
    t0 = time.perf_counter()
    f = W.family(case, pq=True)
    ref, bound, P = W.proxqp_loop(W.Structured(f)), W.bounds(case, pq=True), f.dense_P()
    _proxqp(gpu, case, f, P, ref, bound, t0, "proxqp")
    if case.dtype == "f64" and case.n == W.PQ_BOTH_VARIANTS_N:
        _proxqp(gpu, case, f, P, ref, bound, t0, "proxqp loopVariant 1", variant=1)
    if case.dtype == "f64" and case.n == W.ADAPTIVE_N:
        ra = W.proxqp_loop(W.Structured(f), adpt=True)
        assert ra["firstUpdate"] == W.PERIOD
        _proxqp(gpu, case, f, P, ra, bound, t0, "proxqp adaptive", adpt=True)
