"""The polishing step on the shared-matrix batches on the device (qps_polish_shared, qps_set_shared_polish) through the Python binding, against
oracle/polish_oracle_np.py::Polish per column and a direct solve of K t = g on the active rows (tests/shared_polish_cases.py; tests/test_shared_polish_cpu.py guards
the cases).  Parity tests hand the same (X, Y) to both sides; MINRES iteration counts are never compared with the restatement."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import shared_polish_cases as cases
from infeasibility_cases import case_data

pytestmark = pytest.mark.gpu

BAD_ARGUMENT, UNSUPPORTED = 1, 8
PARITY = cases.PARITY
REPORT_KEYS = ("flag", "refinements", "minresIterations", "numActiveLower", "numActiveUpper", "relres")


def handle(gpu, kind, data, **kw):
    P, A, Q, L, U = data
    if kind == "sparse":
        return gpu.QuadraticProgramSparseSharedBatch(sp.csc_matrix(P), sp.csc_matrix(A), Q, L, U, **kw)
    return gpu.QuadraticProgramSharedBatch(P, A, Q, L, U, **kw)


def check_parity(name, count, X0, Y, X, reps, compared):
    for b in range(count):
        t = cases.direct_of(name, b)
        print(f"{name} count {count} column {b}: flag {reps[b]['flag']} refinements {reps[b]['refinements']} MINRES {reps[b]['minresIterations']} "
              f"relres {reps[b]['relres']:.2e} |x - t| {np.abs(X[b] - t).max():.2e} (input {np.abs(X0[b] - t).max():.2e})")
        assert reps[b]["numActiveLower"] == int((Y[b] < 0).sum()) and reps[b]["numActiveUpper"] == int((Y[b] > 0).sum())
        assert reps[b]["flag"] == 0
        assert np.abs(X[b] - t).max() <= 1e-9
    for b in compared:
        xr, flag, info = cases.restatement(name, b)
        assert reps[b]["flag"] == flag and reps[b]["refinements"] == info["refinements"]
        assert np.abs(X[b] - xr).max() <= 1e-7 * max(1.0, np.abs(xr).max())


@pytest.mark.parametrize("count", [3, 20, 37])
def test_dense_parity_in_every_panel_geometry_of_the_cached_form(gpu, count):
    """One panel, two panels with a ragged second, a pair plus a single."""
    X0, Y = cases.states("dense", count)
    X = X0.copy()
    with handle(gpu, "dense", cases.family("dense", count)) as prob:
        reps = prob.polish(X, Y, **PARITY)
    check_parity("dense", count, X0, Y, X, reps, cases.PARITY_COLUMNS[count])


def test_sparse_parity_on_the_random_family(gpu):
    X0, Y = cases.states("random", 20)
    X = X0.copy()
    with handle(gpu, "sparse", cases.family("random", 20)) as prob:
        reps = prob.polish(X, Y, **PARITY)
    check_parity("random", 20, X0, Y, X, reps, (0, 1, 2, 15, 16, 19))


@pytest.mark.parametrize("kind,name", [("dense", "dense"), ("sparse", "random")])
def test_columns_are_independent_and_runs_repeat(gpu, kind, name):
    """Column b of the count-37 polish equals the same column polished in a handle of its own, bit for bit, x and report (except seconds); a second run of the
    count-37 call is identical."""
    P, A, Q, L, U = cases.family(name, 37)
    X0, Y = cases.states(name, 37)
    with handle(gpu, kind, (P, A, Q, L, U)) as prob:
        X1 = X0.copy(); r1 = prob.polish(X1, Y, **PARITY)
        X2 = X0.copy(); r2 = prob.polish(X2, Y, **PARITY)
    assert np.array_equal(X1, X2) and not np.array_equal(X1, X0)
    assert [[r[k] for k in REPORT_KEYS] for r in r1] == [[r[k] for k in REPORT_KEYS] for r in r2]
    for b in (0, 16, 36):
        with handle(gpu, kind, (P, A, Q[b:b + 1], L[b:b + 1], U[b:b + 1])) as one:
            x = X0[b:b + 1].copy(); r = one.polish(x, Y[b:b + 1], **PARITY)[0]
        assert np.array_equal(x[0], X1[b]), b
        assert [r[k] for k in REPORT_KEYS] == [r1[b][k] for k in REPORT_KEYS], b


def test_staged_kernel_form(gpu):
    """shared_family(2112, 2304, 37): A and A' above the 32 MiB cut, two panels per workgroup; the state is the device's own solve to 1e-4.  On columns 2, 16 and 36
    the polished x is within 4x the restatement's own distance to the direct solve (both stop at the first iterate under the same relative residual, possibly an
    iteration apart) and within a quarter of the ADMM x's distance."""
    k = cases.STAGED
    P, A, Q, L, U = cases.family("staged", k["count"])
    with handle(gpu, "dense", (P, A, Q, L, U)) as prob:
        X0, _, _ = prob.solve(ρ=0.1, ϵAbs=1e-4, ϵRel=1e-4)
        Y = cases.threshold(prob.dual()[1])
        X = X0.copy()
        reps = prob.polish(X, Y, **k["polish"])
    for b in k["columns"]:
        t = cases.direct(P, Q[b], A, L[b], U[b], Y[b])
        d, d0 = np.abs(X[b] - t).max(), np.abs(X0[b] - t).max()
        print(f"staged column {b}: flag {reps[b]['flag']} MINRES {reps[b]['minresIterations']} relres {reps[b]['relres']:.2e} |x - t| {d:.2e} (ADMM {d0:.2e}; "
              f"restatement {cases.STAGED_RESTATEMENT[b]})")
        assert reps[b]["flag"] == 0 and reps[b]["relres"] <= 1e-6
        assert d <= 4 * cases.STAGED_RESTATEMENT[b][1]
        assert d <= d0 / 4
    for b in range(k["count"]):
        assert reps[b]["flag"] in (0, 1)
        if reps[b]["flag"] == 1:
            assert np.array_equal(X[b], X0[b]), b


def test_flags_are_per_column(gpu):
    X0, Y = cases.states("dense", 20)
    with handle(gpu, "dense", cases.family("dense", 20)) as prob:
        X = X0.copy()
        reps = prob.polish(X, Y, numItrPolish=1, δ=1e-6, ϵMinres=1e-9, numItrMinres=cases.FLAG_CAP)
        print("first-call MINRES counts:", [r["minresIterations"] for r in reps])
        for b in range(20):
            if b in cases.FLAG_COLUMNS_OVER:
                assert reps[b]["flag"] == 1 and reps[b]["refinements"] == 1 and np.array_equal(X[b], X0[b]), b
            else:
                assert reps[b]["flag"] == 0 and not np.array_equal(X[b], X0[b]), b
        X = X0.copy()
        reps = prob.polish(X, Y, numItrPolish=10, δ=1e-6, ϵMinres=1e-9, numItrMinres=2)
        assert all(r["flag"] == 1 and r["refinements"] == 1 and r["minresIterations"] == 2 for r in reps) and np.array_equal(X, X0)
        reps = prob.polish(X, Y, numItrPolish=0)
        assert all(r["flag"] == -1 and r["refinements"] == 0 for r in reps) and np.array_equal(X, X0)


@pytest.mark.parametrize("kind,name", [("dense", "dense"), ("sparse", "random")])
def test_chained_form_equals_solve_then_polish(gpu, kind, name):
    kw = dict(ρ=0.1, ϵAbs=1e-4, ϵRel=1e-4)
    pk = dict(numItrPolish=10, δ=1e-6, ϵMinres=1e-9, numItrMinres=4000)
    with handle(gpu, kind, cases.family(name, 20)) as prob:
        X0, f0, i0 = prob.solve(**kw)
        Z0, Y0 = prob.dual()
        assert all(i["polishFlag"] == -1 and i["polishIterations"] == 0 and i["tPolish"] == 0 for i in i0)
        Xs = X0.copy()
        reps = prob.polish(Xs, None, **pk)
        prob.set_polish(True)
        X1, f1, i1 = prob.solve(**kw, **pk)
        Z1, Y1 = prob.dual()
        assert np.array_equal(X1, Xs) and not np.array_equal(X1, X0)
        assert f1 == f0 and [i["iterations"] for i in i1] == [i["iterations"] for i in i0]
        assert [i["polishFlag"] for i in i1] == [r["flag"] for r in reps] and [i["polishIterations"] for i in i1] == [r["minresIterations"] for r in reps]
        assert all(i["tPolish"] > 0 for i in i1)
        assert np.array_equal(Z1, Z0) and np.array_equal(Y1, Y0)              # the stored z and y are those of the unpolished solve
        with pytest.raises(gpu.QpsError) as e:                                # qps_params.polish stays refused
            prob.solve(polish=True, **kw)
        assert e.value.status == UNSUPPORTED and "polish" in e.value.message
        prob.set_polish(False)
        X2, _, i2 = prob.solve(**kw)
        assert np.array_equal(X2, X0) and all(i["polishFlag"] == -1 and i["polishIterations"] == 0 for i in i2)


@pytest.mark.parametrize("kind", ["dense", "sparse"])
def test_chained_form_leaves_an_infeasible_column_alone(gpu, kind):
    """dense-primal-r1 of tests/infeasibility_cases.py: column 4 ends with flag 4 at iteration 100 and keeps polishFlag = -1 and its unpolished x."""
    data = case_data("dense-primal-r1")
    with handle(gpu, kind, data) as prob:
        prob.set_infeasibility()
        X0, f0, _ = prob.solve(ρ=1.0)
        prob.set_polish(True)
        X1, f1, i1 = prob.solve(ρ=1.0, ϵMinres=1e-9, numItrMinres=4000)
    assert [int(f) for f in f1] == [int(f) for f in f0] and int(f1[4]) == 4
    assert i1[4]["polishFlag"] == -1 and i1[4]["polishIterations"] == 0 and np.array_equal(X1[4], X0[4])
    assert all(i1[b]["polishFlag"] in (0, 1) for b in range(6) if b != 4)
    assert any(i1[b]["polishFlag"] == 0 and not np.array_equal(X1[b], X0[b]) for b in range(6) if b != 4)


def test_equilibration_runs_the_step_on_the_scaled_data(gpu):
    data, _, _ = cases.equilibrated()
    X0, Y = cases.states("scrambled", 4)
    X = X0.copy()
    with handle(gpu, "dense", data) as prob:
        prob.set_equilibration(cases.EQUIL_PASSES)
        D, E = prob.equilibration()
        reps = prob.polish(X, Y, **PARITY)
    for b in range(4):
        xr, flag, info = cases.equilibrated_restatement(b, D, E, X0, Y, 4000)
        t = cases.direct_of("scrambled", b)
        print(f"scrambled column {b}: flag {reps[b]['flag']} refinements {reps[b]['refinements']} MINRES {reps[b]['minresIterations']} |x - t| {np.abs(X[b] - t).max():.2e} "
              f"|x - x_r| {np.abs(X[b] - xr).max():.2e} |x_r| {np.abs(xr).max():.2e}")
        assert flag == 0 and reps[b]["flag"] == 0 and reps[b]["refinements"] == info["refinements"]
        assert reps[b]["numActiveLower"] == int((Y[b] < 0).sum()) and reps[b]["numActiveUpper"] == int((Y[b] > 0).sum())
        assert np.abs(X[b] - t).max() <= 1e-9
        assert np.abs(X[b] - xr).max() <= 1e-7 * max(1.0, np.abs(xr).max())


def test_fp32_handle(gpu):
    X0, Y = cases.states("dense", 3)
    X = X0.copy()
    with handle(gpu, "dense", cases.family("dense", 3), dtype="f32") as prob:
        reps = prob.polish(X, Y, numItrPolish=10, δ=1e-6, ϵMinres=1e-3, numItrMinres=4000)
    for b in range(3):
        xr = cases.restatement("dense", b)[0]
        print(f"fp32 column {b}: flag {reps[b]['flag']} MINRES {reps[b]['minresIterations']} |x - x_r| {np.abs(X[b] - xr).max():.2e}")
        assert reps[b]["flag"] == 0
        assert np.abs(X[b] - xr).max() <= 5e-3 * max(1.0, np.abs(xr).max())


def test_sparse_lasso_path_from_the_device_state(gpu):
    """lasso_path(20, 4): the state is the device's own solve under the family-wide rho rule, thresholded; the polished x against a sparse direct solve."""
    P, A, Q, L, U = cases.lasso_path(20, 4)
    with gpu.QuadraticProgramSparseSharedBatch(P, A, Q, L, U) as prob:
        prob.set_adaptive_rho()
        X0, _, _ = prob.solve(ρ=0.1, ϵAbs=1e-4, ϵRel=1e-4)
        Y = cases.threshold(prob.dual()[1])
        X = X0.copy()
        reps = prob.polish(X, Y, numItrPolish=10, δ=1e-6, ϵMinres=1e-9, numItrMinres=4000)
    for b in range(4):
        t = cases.direct(sp.csc_matrix(P), Q[b], A, L[b], U[b], Y[b])
        print(f"lasso column {b}: flag {reps[b]['flag']} MINRES {reps[b]['minresIterations']} |x - t| {np.abs(X[b] - t).max():.2e} (ADMM {np.abs(X0[b] - t).max():.2e})")
        assert reps[b]["flag"] == 0
        assert np.abs(X[b] - t).max() <= 1e-9 * max(1.0, np.abs(t).max())


def test_refusals(gpu):
    from quadraticprogramsolver_amd import _lib
    L_ = _lib.lib()
    P, A, Q, L, U = cases.family("dense", 3)
    X0, Y = cases.states("dense", 3)
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    p = _lib.default_params()
    with gpu.QuadraticProgram(P, Q[0], A, L[0], U[0]) as one, gpu.QuadraticProgramBatch([(P, Q[b], A, L[b], U[b]) for b in range(2)]) as batch:
        x = X0[:2].copy(); reps = (_lib.QpsPolishReport * 2)()
        for h in (one._h, batch._h):
            assert L_.qps_polish_shared(h, ptr(x), ptr(Y), C.byref(p), reps) == UNSUPPORTED and b"shared-matrix batch" in L_.qps_last_error(h)
            assert L_.qps_set_shared_polish(h, 1) == UNSUPPORTED and b"shared-matrix batch" in L_.qps_last_error(h)
        assert np.array_equal(x, X0[:2])
    with handle(gpu, "dense", (P, A, Q, L, U)) as prob:
        bad = Y.copy(); bad[1, 5] = np.nan
        X = X0.copy()
        with pytest.raises(gpu.QpsError) as e:
            prob.polish(X, bad, **PARITY)
        assert e.value.status == BAD_ARGUMENT and np.array_equal(X, X0)
        X[2, 0] = np.inf
        with pytest.raises(gpu.QpsError) as e:
            prob.polish(X, Y, **PARITY)
        assert e.value.status == BAD_ARGUMENT
        assert L_.qps_set_shared_polish(prob._h, 2) == BAD_ARGUMENT
        assert L_.qps_polish_shared(prob._h, None, None, C.byref(p), None) == BAD_ARGUMENT
        with pytest.raises(ValueError):
            prob.polish(X0[:2].copy(), Y)
        X = X0.copy()
        reps = prob.polish(X, Y, **PARITY)                                    # the handle stays usable
        assert all(r["flag"] == 0 for r in reps)
        Xf = X0.copy()
        reps = prob.polish(Xf)                                                # before any solve and without y: y = 0, every mask empty, P t = -q
        for b in range(3):
            assert reps[b]["flag"] == 0 and reps[b]["numActiveLower"] == 0 and reps[b]["numActiveUpper"] == 0
            # the last MINRES call ended with |rhs - (P + delta I) tt| <= epsMinres |rhs|, |rhs| <= |q|, and -q - P (t + tt) = (rhs - (P + delta I) tt) + delta tt
            res = np.linalg.norm(P @ Xf[b] + Q[b])
            print(f"unconstrained column {b}: MINRES {reps[b]['minresIterations']} |P x + q| {res:.2e} |q| {np.linalg.norm(Q[b]):.2e}")
            assert res <= 1e-6 * (np.linalg.norm(Q[b]) + np.linalg.norm(Xf[b]))
