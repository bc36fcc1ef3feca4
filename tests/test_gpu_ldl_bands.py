"""The sparse direct KKT plugin (k_ldl.hip, HipLdlInit / HipLdl) in every lane-group band of its two triangular sweeps, both types: every case of
tests/ldl_band_cases.py through the plugin pair in isolation -- one linear solve shows a wrong partial sum undiluted by ADMM -- against a refined fp64
solve of the same K.  The case id names the forms the case reaches (k_ldl_fwd / k_ldl_bwd<T, LPR> per level, the tail rows), as tests/test_ldl_bands_cpu.py
holds them against the analysis; the handle's own analysis must report the case's shape.  Bounds (ldl_band_cases.bounds): fp64 1e-9 relative on x~ and z~;
fp32 8 x the recorded error of the float32 emulation of the same case and step.  The four steps re-factorise twice (k_ldl_level_diag / k_ldl_level_offdiag,
on the dense patterns with both orders of its sorted-list intersection), so the numeric phase, the signed dense tail (cholesky_signed, k_ldl_mul_sign) and
the K-split Schur complement (k_ldl_densify, the batched GEMM, k_ldl_sub_slabs with a partial last slice) are held to the same bounds.  Run with -s for the
figures of every step."""
import ctypes as C

import numpy as np
import pytest

import ldl_band_cases as B

pytestmark = pytest.mark.gpu

CASE_IDS = [B.case_label(c).replace(" ", "-") for c in B.CASES]


def set_limits(monkeypatch, case):
    for k, v in B.case_env(case).items():
        monkeypatch.setenv(k, v)                         # read when the handle analyses its KKT matrix (first use of the plugin)
    monkeypatch.delenv("QPS_LDL_MAX_LEVELS", raising=False)
    monkeypatch.delenv("QPS_LDL_PANEL_SPR", raising=False)


def analysis_report(P, A):
    """qps_ldl_analyze of the product library under the current QPS_LDL_* limits: what the handle's plugin will hold."""
    from quadraticprogramsolver_amd import _lib
    arrs = [np.ascontiguousarray(a, dtype=np.int64) for a in (P.indptr, P.indices, A.indptr, A.indices)]
    rep = _lib.QpsLdlReport()
    _lib.check(_lib.lib().qps_ldl_analyze(P.shape[0], A.shape[0], *[a.ctypes.data_as(C.POINTER(C.c_int64)) for a in arrs], 0, None, C.byref(rep)))
    return rep.numRows, rep.numSparseColumns, rep.tailSize, rep.numSparseLevels


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("case", B.CASES, ids=CASE_IDS)
def test_plugin_pair_in_every_band(gpu, monkeypatch, case, dtype):
    set_limits(monkeypatch, case)
    P, q, A, l, u = B.problem(case.name)
    n, m = P.shape[0], A.shape[0]
    assert analysis_report(P, A) == (case.shape[0], case.shape[1], case.shape[2], case.shape[4])
    figs = []
    with gpu.QuadraticProgram(P, q, A, l, u, linsys="ldl", dtype=dtype) as prob:
        prob.linsys_init(B.STEPS[0][1], B.SIGMA)
        for step, (changed, rho) in enumerate(B.STEPS):
            x, z, y = B.step_inputs(case.name)[step]
            xx, zz = np.zeros(n), np.zeros(m)
            prob.linsys_solve(x, z, y, rho, B.SIGMA, changed, xx, zz)
            rx, rz = B.reference(case.name, step)
            figs.append((B.rel(xx, rx), B.rel(zz, rz)) + B.bounds(case.name, step, dtype))
    for step, (ex, ez, bx, bz) in enumerate(figs):
        print(f"{B.case_label(case)} {dtype} step {step} changedRho {int(B.STEPS[step][0])} rho {B.STEPS[step][1]:g}: rel x~ {ex:.2e} / {bx:.2e} ({ex / bx:.2f}) "
              f"z~ {ez:.2e} / {bz:.2e} ({ez / bz:.2f})")
    for step, (ex, ez, bx, bz) in enumerate(figs):
        assert ex <= bx and ez <= bz, (case.name, dtype, step, ex, bx, ez, bz)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", B.REPEAT_CASES)
def test_solves_repeat_bit_for_bit(gpu, monkeypatch, name, dtype):
    """Fixed summation order, no atomics: the same inputs give the same bits, also across a re-factorisation at the same rho."""
    case = B.find(name)
    set_limits(monkeypatch, case)
    P, q, A, l, u = B.problem(name)
    x, z, y = B.step_inputs(name)[1]
    rho = B.STEPS[1][1]
    out = []
    with gpu.QuadraticProgram(P, q, A, l, u, linsys="ldl", dtype=dtype) as prob:
        prob.linsys_init(rho, B.SIGMA)
        for changed in (False, False, True):
            xx, zz = np.zeros(P.shape[0]), np.zeros(A.shape[0])
            prob.linsys_solve(x, z, y, rho, B.SIGMA, changed, xx, zz)
            out.append((xx, zz))
    assert np.abs(out[0][0]).max() > 0 and np.abs(out[0][1]).max() > 0
    for xx, zz in out[1:]:
        assert np.array_equal(xx, out[0][0]) and np.array_equal(zz, out[0][1])


@pytest.mark.parametrize("name", B.PANEL_CASES)
def test_panel_sweeps_pick_their_strips_per_level(gpu, c_oracle, monkeypatch, name):
    """The panel forms k_ldl_fwd_panel / k_ldl_bwd_panel<T, SPR> with QPS_LDL_PANEL_SPR unset, so that pick_panel_spr chooses per level (the three cases
    reach SPR 1, 4 and 16 between them: CPU guard): 17 columns = two panels, the second with one live column; 20 fixed iterations (a check every 10, so that the residuals of the last
    check are compared too) in fp64 against the C oracle's sparse L D L' per column, at the bounds of check_fixed_k of tests/test_gpu_sparse_shared_batch.py."""
    case = B.find(name)
    set_limits(monkeypatch, case)
    P, A, Q, L, U = B.panel_family(name)
    perm = c_oracle.kkt_ordering(P, A)
    with gpu.QuadraticProgramSparseSharedBatch(P, A, Q, L, U) as prob:
        X, flags, infos = prob.solve(numIterations=B.PANEL_K, numItrConv=B.PANEL_PERIOD, ϵAbs=0.0, ϵRel=0.0, ρ=0.1)
        Z, Y = prob.dual()
    assert X.shape == Q.shape and Z.shape == L.shape and Y.shape == L.shape
    tol, figs = 1e-9, []
    for b in range(B.PANEL_COUNT):
        xo, io = c_oracle.solve(P, Q[b], A, L[b], U[b], perm=perm, rho=0.1, numIterations=B.PANEL_K, numItrConv=B.PANEL_PERIOD, epsAbs=0.0, epsRel=0.0, linsys=c_oracle.KIND_KKT_LDL_SPARSE)
        fig = (B.rel(X[b], xo), B.rel(Z[b], io["z"]), B.rel(Y[b], io["y"]), abs(infos[b]["resPrim"] - io["resPrim"]) / max(1.0, io["resPrim"]),
               abs(infos[b]["resDual"] - io["resDual"]) / max(1.0, io["resDual"]))
        figs.append(fig)
        print(f"{name} column {b}: rel x {fig[0]:.2e} z {fig[1]:.2e} y {fig[2]:.2e} dresPrim {fig[3]:.2e} dresDual {fig[4]:.2e}")
    for b, fig in enumerate(figs):
        assert flags[b] == gpu.ConvergenceFlag.convNumItr and infos[b]["iterations"] == B.PANEL_K
        assert fig[0] <= tol and fig[1] <= tol and fig[2] <= 10 * tol, (name, b, fig)
        assert fig[3] <= tol and fig[4] <= 10 * tol, (name, b, fig)                    # (a NaN, no check run on one side, fails here)
