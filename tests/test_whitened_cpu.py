"""CPU companion of tests/test_gpu_whitened.py: the whitened recurrences (u = W t, p = W x, a = A x carried by its own recurrence, x / x - xp / A'y as
three products with L; tests/whitened_cases.py: whitened_loop) held to oracle/qps_oracle_np.py on the cases of the GPU test, with the bounds the GPU
test uses.  Every figure is printed before its assertion (run with -s).

Measured (fixed K = 60, check every 10), worst over the four shapes and the off-default (α, σ), all at (4100, 70): x 1.0e-14, z 2.5e-13, y 2.9e-14,
resPrim 8.5e-14, resDual 2.0e-12; the carried a against A x: 4.4e-14.  To ϵ = 1e-6: both stop with flag 3 at iteration 2350, one check earlier the larger
residual stands at 1.069 of its tolerance.  Stall stop: flag 2 at iteration 500 on both sides, the step 1.089e-6 one check earlier and 7.84e-7 at the stop
against ϵAdmm = 1e-6; x 2.5e-14, residuals within 4.1e-13."""
import numpy as np
import pytest

import whitened_cases as W
from loop_param_cases import TOL

BOUND = TOL["f64"]


def np_reference(np_oracle, shape, x0=None, stall=False, **p):
    P, q, A, l, u = W.problem(shape, stall)
    x = np.zeros(shape[0]) if x0 is None else np.array(x0)
    info = {}
    flag = np_oracle.SolveQuadraticProgramRefLoop(x, P, q, A, l, u, np_oracle.RedCholInit, np_oracle.RedChol, numIterations=p["numIterations"],
                                                  ϵAbs=p["epsAbs"], ϵRel=p["epsRel"], ρ=p["rho"], σ=p["sigma"], α=p["alpha"], numItrConv=p["numItrConv"],
                                                  info=info)
    return dict(x=x, z=info["z"], y=info["y"], resPrim=info["res_prim"], resDual=info["res_dual"], convFlag=int(flag), iterations=info["iterations"])


def hold(tag, got, want):
    for f in W.FIELDS:
        d = W.rel(got[f], want[f])
        print(f"{tag}: {f} {d:.2e} (bound {BOUND[f]:.0e})")
        assert d <= BOUND[f], (tag, f, d)


@pytest.mark.parametrize("shape", W.SHAPES, ids=W.IDS)
def test_whitened_recurrence_matches_numpy_oracle(np_oracle, shape):
    p = W.fixed_k()
    got = W.whitened_loop(*W.problem(shape), **p)
    hold(f"{shape} fixed K", got, np_reference(np_oracle, shape, **p))
    d = W.rel(got["a"], got["A_x"])
    print(f"{shape}: carried a against A x {d:.2e}")
    assert d <= BOUND["z"] and got["iterations"] == W.K and got["convFlag"] == 1


@pytest.mark.parametrize("alpha,sigma", W.OFF_DEFAULT)
def test_off_default_alpha_sigma_and_start(np_oracle, alpha, sigma):
    shape = W.SHAPES[0]
    p = W.fixed_k(alpha=alpha, sigma=sigma)
    x0 = W.start(shape)
    hold(f"{shape} alpha={alpha} sigma={sigma} x0 != 0", W.whitened_loop(*W.problem(shape), x0, **p), np_reference(np_oracle, shape, x0, **p))


def test_stop_by_tolerance_at_the_oracles_iteration(np_oracle):
    """Fixed ρ to ϵ = 1e-6: flag and stopping iteration equal the oracle's, and the stop has margin: at the check before it the test is missed by a
    factor, not by rounding (the whitened residuals differ from the reference's by 1e-12 at most)."""
    shape = W.SHAPES[0]
    want = np_reference(np_oracle, shape, **W.TO_EPS)
    got = W.whitened_loop(*W.problem(shape), **W.TO_EPS)
    print(f"{shape} to eps: oracle flag {want['convFlag']} at {want['iterations']}, whitened flag {got['convFlag']} at {got['iterations']}")
    assert (got["convFlag"], got["iterations"]) == (want["convFlag"], want["iterations"]) and want["convFlag"] == 3
    assert want["iterations"] < W.TO_EPS["numIterations"]
    hold(f"{shape} to eps", got, want)
    before = np_reference(np_oracle, shape, **dict(W.TO_EPS, numIterations=want["iterations"] - W.TO_EPS["numItrConv"], epsAbs=0.0, epsRel=0.0))
    P, q, A, l, u = W.problem(shape)
    Ax, Px, Aty = A @ before["x"], P @ before["x"], A.T @ before["y"]
    inf = lambda v: float(np.abs(v).max())
    eps = W.TO_EPS["epsAbs"]
    miss = max(before["resPrim"] / (eps + eps * max(inf(Ax), inf(before["z"]))), before["resDual"] / (eps + eps * max(inf(Px), inf(Aty), inf(q))))
    print(f"{shape} to eps: one check earlier the larger residual stands at {miss:.3f} of its tolerance")
    assert miss > 1.0 + 1e-6


def test_stall_stop_is_decided_by_the_step_norm(np_oracle):
    """Equality rows nothing satisfies: convAdmm at the oracle's iteration, decided by |x - xp| = |L (p - pp)| alone (|z - zp| = 0), with margin on both
    sides of ϵAdmm: the step one check earlier is above it, the stopping one below, by far more than rounding."""
    shape = W.SHAPES[0]
    want = np_reference(np_oracle, shape, stall=True, **W.STALL)
    got = W.whitened_loop(*W.problem(shape, stall=True), **W.STALL)
    eps_admm = min(W.STALL["epsAbs"], W.STALL["epsRel"]) * 1e-2
    print(f"{shape} stall: oracle flag {want['convFlag']} at {want['iterations']}, whitened flag {got['convFlag']} at {got['iterations']}; step at the last two "
          f"checks {got['steps'][-2]:.3e}, {got['steps'][-1]:.3e} against {eps_admm:.0e}")
    assert (got["convFlag"], got["iterations"]) == (want["convFlag"], want["iterations"]) and want["convFlag"] == 2
    assert W.STALL["numItrConv"] < want["iterations"] < W.STALL["numIterations"]
    assert got["steps"][-2] > 1.01 * eps_admm and got["steps"][-1] < 0.99 * eps_admm
    hold(f"{shape} stall", got, want)
