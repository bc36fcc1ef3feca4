"""Per-column infeasibility certificates of the shared-matrix batches on the device (qps_set_shared_infeasibility, qps_get_shared_certificate), through the Python
wrapper.  Every column behaves as the numpy restatement of tests/infeasibility_cases.py -- its reduced Cholesky form for the dense handle, its dense KKT form for
the sparse one -- and every returned certificate is also checked without trusting the restatement: the rule's inequalities are recomputed in numpy float64 from
the certificate and the original P, A, q, l, u.  eps = 1e-6, numItrConv = 25, eps_p = eps_d = 1e-4; the cases and their CPU figures are the table there, and
tests/test_infeasibility_cpu.py keeps every decision of every case 2 % away from a rounding edge.

Bounds are those of tests/test_gpu_family_rho.py for the same kind of family: dense fp64 and sparse random 1e-9 relative on x and z, 1e-8 on y; lasso 1e-6 / 1e-5.
A certificate is a difference of two consecutive iterates and inherits their error amplified by the cancellation: its relative bound is the family's y bound times
||y|| / ||dyh|| (flag 4) or the x bound times ||x|| / ||dx|| (flag 5), norms from the restatement."""
import ctypes
import functools

import numpy as np
import pytest

from family_rho_cases import case_data as family_case_data
from infeasibility_cases import CASES, DUAL_INFEASIBLE, EPS, EPS_INF, NUM_ITR_CONV, PRIM_INFEASIBLE, case_data, case_run, certificate_holds
from test_gpu_parity import rel

pytestmark = pytest.mark.gpu

BAD_ARGUMENT, UNSUPPORTED = 1, 8
INFO_KEYS = ("iterations", "numRefactor", "rhoFinal", "rhoProposed", "resPrim", "resDual")


@functools.lru_cache(maxsize=None)
def data(name):
    return case_data(name)


def _make(gpu, sparse, P, A, Q, L, U, **kw):
    return (gpu.QuadraticProgramSparseSharedBatch if sparse else gpu.QuadraticProgramSharedBatch)(P, A, Q, L, U, **kw)


def _solve_kw(name):
    s = CASES[name]["solve"]
    kw = dict(ϵAbs=EPS, ϵRel=EPS, numItrConv=NUM_ITR_CONV, ρ=s["rho"], numIterations=s.get("numIterations", 5000))
    if "fctrRho" in s:
        kw["fctrΡ"] = s["fctrRho"]
    return kw


def _open(gpu, name, *, on=True, dtype="f64", columns=None):
    """The handle of a case with the case's options set; ``columns``: only those columns (a batch of its own)."""
    c = CASES[name]
    P, A, Q, L, U = data(name)
    if columns is not None:
        Q, L, U = Q[columns], L[columns], U[columns]
    prob = _make(gpu, c["handle"] == "sparse", P, A, Q, L, U, dtype=dtype)
    if c.get("passes"):
        prob.set_equilibration(c["passes"])
    if c["solve"].get("adaptive"):
        prob.set_adaptive_rho()
    if on:
        prob.set_infeasibility(c.get("eps_p", EPS_INF), c.get("eps_d", EPS_INF))
    return prob


def _run(prob, **kw):
    X, flags, infos = prob.solve(**kw)
    Z, Y = prob.dual()
    DY, DX = prob.certificate()
    return X, Z, Y, [int(f) for f in flags], infos, DY, DX


def _same(a, b):
    return (all(np.array_equal(p, q) for p, q in zip(a[:3], b[:3])) and a[3] == b[3] and np.array_equal(a[5], b[5]) and np.array_equal(a[6], b[6])
            and [[i[k] for k in INFO_KEYS] for i in a[4]] == [[i[k] for k in INFO_KEYS] for i in b[4]])


def _relv(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def compare_with_restatement(name, run, ref, xz_tol, y_tol):
    X, Z, Y, flags, infos, DY, DX = run
    figs = []
    for b, col in enumerate(ref["columns"]):
        fig = [rel(X[b], col["x"]), rel(Z[b], col["z"]), rel(Y[b], col["y"]), 0.0, 0.0]
        if col["convFlag"] == PRIM_INFEASIBLE:
            fig[3:] = _relv(DY[b], col["dy"]), y_tol * np.abs(col["y"]).max() / np.abs(col["dy"]).max()
        elif col["convFlag"] == DUAL_INFEASIBLE:
            fig[3:] = _relv(DX[b], col["dx"]), xz_tol * np.abs(col["x"]).max() / np.abs(col["dx"]).max()
        print(f"{name} column {b}: flag {flags[b]}/{col['convFlag']} iterations {infos[b]['iterations']}/{col['iterations']} rel x {fig[0]:.2e} z {fig[1]:.2e} "
              f"y {fig[2]:.2e} certificate {fig[3]:.2e} (bound {fig[4]:.2e})")
        figs.append(fig)
    for b, (col, fig) in enumerate(zip(ref["columns"], figs)):
        assert flags[b] == col["convFlag"] and infos[b]["iterations"] == col["iterations"] and infos[b]["numRefactor"] == col["numRefactor"], (name, b)
        assert fig[0] <= xz_tol and fig[1] <= xz_tol and fig[2] <= y_tol, (name, b, fig)
        assert fig[3] <= fig[4], (name, b, fig)
        if col["convFlag"] != PRIM_INFEASIBLE:
            assert not DY[b].any(), (name, b)
        if col["convFlag"] != DUAL_INFEASIBLE:
            assert not DX[b].any(), (name, b)


def assert_certificates_hold(name, run, eps=EPS_INF):
    """The test that does not trust the restatement: the rule's inequalities in numpy float64 from the returned certificate and the original data."""
    P, A, Q, L, U = data(name)
    for b, flag in enumerate(run[3]):
        assert certificate_holds(P, A, Q[b], L[b], U[b], run[5][b], run[6][b], flag, eps, eps), (name, b, flag)


# ---------------------------------------------------------------------------------------------------------------------
# 1. every case: flags, stopping iterations, iterates and certificates against the restatement; the certificates on their own
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_case_matches_the_restatement_and_its_certificates_hold(gpu, name):
    c = CASES[name]
    xz_tol, y_tol = (1e-6, 1e-5) if c.get("lasso") else (1e-9, 1e-8)
    with _open(gpu, name) as prob:
        DY0, DX0 = prob.certificate()
        assert not DY0.any() and not DX0.any() and DY0.shape == data(name)[3].shape and DX0.shape == data(name)[2].shape          # before any solve: zeros
        run = _run(prob, **_solve_kw(name))
    assert run[3] == c["flags"] and [i["iterations"] for i in run[4]] == c["iterations"]
    compare_with_restatement(name, run, case_run(name), xz_tol, y_tol)
    assert_certificates_hold(name, run, c.get("eps_p", EPS_INF))


def test_known_answers_have_the_expected_support_and_signs(gpu):
    with _open(gpu, "known-primal") as prob:
        run = _run(prob, **_solve_kw("known-primal"))
    dy = run[5][1]
    print("known-primal: dyh of column 1", dy)
    assert run[3] == [3, PRIM_INFEASIBLE] and dy[0] < 0 < dy[1]                          # x1 >= 1 pushes down, x1 <= 0 pushes up, |x2| <= 1 takes no part:
    assert max(abs(dy[0] + dy[1]), abs(dy[2])) <= 1e-4 * np.abs(dy).max()                # A'dyh = (dyh_0 + dyh_1, dyh_2) is below eps_p ||dyh||
    assert not run[5][0].any() and not run[6].any()
    with _open(gpu, "known-dual") as prob:
        run = _run(prob, **_solve_kw("known-dual"))
    dx = run[6][1]
    print("known-dual: dx of column 1", dx)
    assert run[3] == [3, DUAL_INFEASIBLE] and dx[0] > 0 and abs(dx[1]) <= 1e-4 * dx[0] and not run[6][0].any() and not run[5].any()


# ---------------------------------------------------------------------------------------------------------------------
# 2. off is the untouched path; on with every column feasible changes nothing
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
def test_off_is_untouched_and_on_changes_nothing_for_feasible_columns(gpu, sparse):
    """shared96-eq-f5 (dense, equality rho scale) and lasso10-f4 (sparse) of tests/family_rho_cases.py, under the family rule: a handle that never saw the option,
    one with set_infeasibility(None), one switched on and off again, and one with the option on give bit-identical X, Z, Y, flags and info fields -- every column
    is feasible -- and the option stays with the handle across solves."""
    name = "lasso10-f4" if sparse else "shared96-eq-f5"
    P, A, Q, L, U, s, f = family_case_data(name)
    fixed = dict(numIterations=300, fctrΡ=f, ϵAbs=EPS, ϵRel=EPS, ρ=0.1, numItrConv=NUM_ITR_CONV)

    def fresh():
        prob = _make(gpu, sparse, P, A, Q, L, U)
        if s is not None:
            prob.set_rho_scale(s)
        prob.set_adaptive_rho()
        return prob
    with fresh() as never:
        plain = _run(never, **fixed)
    with fresh() as prob:
        prob.set_infeasibility(None, None)
        none = _run(prob, **fixed)
        prob.set_infeasibility()
        on = _run(prob, **fixed)
        again = _run(prob, **fixed)
        prob.set_infeasibility(0, False)
        back = _run(prob, **fixed)
    assert max(i["numRefactor"] for i in plain[4]) >= 1 and set(plain[3]) <= {1, 2, 3}
    assert _same(none, plain) and _same(back, plain)
    assert _same(on, plain) and _same(again, plain)
    assert not plain[5].any() and not plain[6].any()


# ---------------------------------------------------------------------------------------------------------------------
# 3. a column of a batch is the same data in a batch of one, certificate included
# ---------------------------------------------------------------------------------------------------------------------
def test_an_infeasible_column_alone_equals_its_column_in_the_batch(gpu):
    name = "multi-r05"
    with _open(gpu, name) as prob:
        whole = _run(prob, **_solve_kw(name))
    for b in (3, 17):                                          # one in each panel; 17 sits in the ragged one
        with _open(gpu, name, columns=[b]) as one:
            alone = _run(one, **_solve_kw(name))
        assert alone[3] == [PRIM_INFEASIBLE] and alone[5].any()
        assert all(np.array_equal(alone[k][0], whole[k][b]) for k in (0, 1, 2, 5, 6)), b
        assert [alone[4][0][k] for k in INFO_KEYS] == [whole[4][b][k] for k in INFO_KEYS]


def test_sparse_infeasible_column_alone_equals_its_column_in_the_batch(gpu):
    name = "sparse-primal-r1"
    with _open(gpu, name) as prob:
        whole = _run(prob, **_solve_kw(name))
    with _open(gpu, name, columns=[3]) as one:
        alone = _run(one, **_solve_kw(name))
    assert alone[3] == [PRIM_INFEASIBLE] and alone[5].any()
    assert all(np.array_equal(alone[k][0], whole[k][3]) for k in (0, 1, 2, 5, 6))
    assert [alone[4][0][k] for k in INFO_KEYS] == [whole[4][3][k] for k in INFO_KEYS]


# ---------------------------------------------------------------------------------------------------------------------
# 4. what it is for
# ---------------------------------------------------------------------------------------------------------------------
def test_an_infeasible_column_no_longer_holds_the_batch_and_steers_rho(gpu):
    """steer-primal-f5: the family rule on, column 5 infeasible.  Without the option it ends with flag 1 at numIterations and the feasible columns stop where the
    restatement says they do with that column steering rho; with it the batch's longest run is below numIterations and every feasible column matches the
    restatement run with the option on (test 1 compares that run's iterates)."""
    name = "steer-primal-f5"
    c, kw = CASES[name], _solve_kw(name)
    with _open(gpu, name, on=False) as prob:
        off = _run(prob, **kw)
        prob.set_infeasibility()
        on = _run(prob, **kw)
    ref_off, ref_on = case_run(name, on=False), case_run(name)
    print("off:", list(zip(off[3], [i["iterations"] for i in off[4]])), " on:", list(zip(on[3], [i["iterations"] for i in on[4]])))
    assert off[3][5] == 1 and off[4][5]["iterations"] == kw["numIterations"]
    assert off[3] == c["off"]["flags"] == [k["convFlag"] for k in ref_off["columns"]]
    assert [i["iterations"] for i in off[4]] == c["off"]["iterations"] == [k["iterations"] for k in ref_off["columns"]]
    assert [i["numRefactor"] for i in off[4]] == [k["numRefactor"] for k in ref_off["columns"]]
    assert max(i["iterations"] for i in on[4]) < kw["numIterations"]
    compare_with_restatement(name, on, ref_on, 1e-9, 1e-8)
    assert all(fl == 3 for fl in on[3][:5]) and on[3][5] == PRIM_INFEASIBLE
    assert max(i["numRefactor"] for i in on[4]) < max(i["numRefactor"] for i in off[4])


# ---------------------------------------------------------------------------------------------------------------------
# 5. fp32
# ---------------------------------------------------------------------------------------------------------------------
def test_fp32_flags_the_same_column(gpu):
    """dense-primal-r1-e3 on an fp32 handle: eps_p = eps_d = 1e-3, column 4 gets flag 4 as in fp64 and its certificate passes the numpy validity test at 10 eps.
    The thresholds come from the format: dy = y - y_prev is formed in fp32 with an absolute error of half an ulp of y, 6e-8 ||y||; y of an infeasible column grows by
    dy per iteration, so after k iterations that is 6e-8 k ||dy||, and A' (||A||_2 ~ sqrt(m) + sqrt(n) = 22 here) carries it into ||A'dyh|| / ||dyh|| as 1.3e-4 at
    k = 100 -- above 1e-4, which an fp32 handle therefore cannot decide on this family (measured: the quotient bottoms out at 2e-4 and the column runs to
    numIterations), and a decade below 1e-3.  fp32 iterates carry ~1e-3 relative error, so a comparison can cross its threshold one check earlier or later than
    in fp64: exactly one check (numItrConv iterations) either way is allowed for the stopping iteration, no more."""
    name = "dense-primal-r1-e3"
    eps = CASES[name]["eps_p"]
    with _open(gpu, name, dtype="f32") as prob:
        run = _run(prob, **_solve_kw(name))
    it = run[4][4]["iterations"]
    print("fp32: flags", run[3], "iterations", [i["iterations"] for i in run[4]], "against", CASES[name]["iterations"])
    assert run[3][4] == PRIM_INFEASIBLE == CASES[name]["flags"][4] and abs(it - CASES[name]["iterations"][4]) <= NUM_ITR_CONV
    assert all(fl in (1, 2, 3) for b, fl in enumerate(run[3]) if b != 4)
    P, A, Q, L, U = data(name)
    assert certificate_holds(P, A, Q[4], L[4], U[4], run[5][4], run[6][4], PRIM_INFEASIBLE, 10 * eps, 10 * eps)
    assert not run[6].any() and not np.delete(run[5], 4, axis=0).any()


# ---------------------------------------------------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
def test_bad_values_are_refused_and_the_handle_keeps_its_setting(gpu, sparse):
    from quadraticprogramsolver_amd import _lib
    name = "sparse-primal-r1" if sparse else "dense-primal-r1"
    fn = _lib.lib().qps_set_shared_infeasibility
    with _open(gpu, name) as prob:
        ok = _run(prob, **_solve_kw(name))
        for ep, ed in ((-1e-4, 1e-4), (1e-4, -1.0), (float("nan"), 1e-4), (1e-4, float("inf")), (float("-inf"), 0.0)):
            assert fn(prob._h, ep, ed) == BAD_ARGUMENT
            with pytest.raises(gpu.QpsError) as e:
                prob.set_infeasibility(ep, ed)
            assert e.value.status == BAD_ARGUMENT and "qps_set_shared_infeasibility" in e.value.message
        assert _same(_run(prob, **_solve_kw(name)), ok) and PRIM_INFEASIBLE in ok[3]      # still on, with the previous tolerances
        prob.set_infeasibility(None, EPS_INF)                  # the primal test alone off: the column is not flagged
        assert PRIM_INFEASIBLE not in _run(prob, numIterations=150, ϵAbs=EPS, ϵRel=EPS, ρ=1.0)[3]


def test_other_handles_are_unsupported(gpu):
    from quadraticprogramsolver_amd import _lib
    P, A, Q, L, U = data("dense-primal-r1")
    L_ = _lib.lib()
    dy, dx = np.zeros(A.shape[0]), np.zeros(A.shape[1])
    ptr = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    with gpu.QuadraticProgram(P, Q[0], A, L[0], U[0]) as one:
        assert L_.qps_set_shared_infeasibility(one._h, 1e-4, 1e-4) == UNSUPPORTED and b"shared-matrix batch" in L_.qps_last_error(one._h)
        assert L_.qps_get_shared_certificate(one._h, ptr(dy), ptr(dx)) == UNSUPPORTED and b"shared-matrix batch" in L_.qps_last_error(one._h)
        assert L_.qps_set_shared_infeasibility(one._h, -1.0, 1e-4) == BAD_ARGUMENT
    with gpu.QuadraticProgramBatch([(P, Q[b], A, L[b], U[b]) for b in range(2)]) as batch:
        assert L_.qps_set_shared_infeasibility(batch._h, 1e-4, 1e-4) == UNSUPPORTED and b"shared-matrix batch" in L_.qps_last_error(batch._h)
        assert L_.qps_get_shared_certificate(batch._h, None, None) == UNSUPPORTED and b"shared-matrix batch" in L_.qps_last_error(batch._h)
