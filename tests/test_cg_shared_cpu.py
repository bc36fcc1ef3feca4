"""CPU-only checks of the matrix-free CG shared-matrix batch boundary (qps_create_csc_shared_batch_cg) and guards on the cases of
tests/test_gpu_cg_shared_batch.py: the symbol is declared, exported and bound; arguments are tested in the order of qps_create_csc_shared_batch, with its
statuses and texts, before a device is needed; with the numpy oracle's LinOpCg at the tight inner tolerance no compared column runs into numItrPcg and no
decision of any check hangs on less than 1 %; the restated dispatch of k_cg_panel.hip reaches every strip count and a ragged last workgroup."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import cg_shared_cases as cases
import family_rho_cases as frc
from cg_shared_cases import COUNT, EPS_PCG_TIGHT, ITR_PCG_TIGHT, RANDOM_FAMILY_ORACLE_ITERATIONS, RHO, banded_family, random_family
from test_sparse_shared_cpu import _d, _i, _problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME, TWIN = "qps_create_csc_shared_batch_cg", "qps_create_csc_shared_batch"
BAD_ARGUMENT, BAD_DIMENSION, NOT_FINITE, NO_DEVICE, UNSUPPORTED = 1, 2, 3, 7, 8
MARGIN = 0.01


def _create(L, name, a, base=0, dtype=0, out=True):
    h = C.c_void_p()
    (Pcp, Pri, Pnz), (Acp, Ari, Anz) = a["P"], a["A"]
    rc = getattr(L, name)(a["count"], a["n"], a["m"], _i(Pcp), _i(Pri), _d(Pnz), _i(Acp), _i(Ari), _d(Anz), _d(a["q"]), _d(a["l"]), _d(a["u"]), base, dtype, 0,
                          C.byref(h) if out else None)
    msg = (L.qps_last_error(None) or b"").decode()
    if h.value:
        L.qps_destroy(h)
    return rc, msg


def test_symbol_is_declared_exported_and_bound(qps):
    from quadraticprogramsolver_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qps.h")).read(), flags=re.S)
    assert re.search(r"\b%s\s*\(" % NAME, header), f"{NAME} is not declared in include/qps.h"
    assert NAME in _lib.EXPORTED_SYMBOLS
    assert hasattr(C.CDLL(_lib.LIB_PATH), NAME), f"{NAME} is not exported by the library"
    fn = getattr(_lib.lib(), NAME)
    assert fn.restype is C.c_int32 and len(fn.argtypes) == 16 and fn.argtypes == getattr(_lib.lib(), TWIN).argtypes


def test_python_class_exists_and_validates_shapes(qps):
    assert hasattr(qps, "QuadraticProgramCgSharedBatch") and "QuadraticProgramCgSharedBatch" in qps.__all__
    assert issubclass(qps.QuadraticProgramCgSharedBatch, qps.QuadraticProgramSharedBatch)
    P, A, Q, L, U = random_family(3)
    with pytest.raises(ValueError):
        qps.QuadraticProgramCgSharedBatch(P, A, Q, L[:, :-1], U)
    with pytest.raises(ValueError):
        qps.QuadraticProgramCgSharedBatch(P, A, Q[:, :-1], L, U)


def test_arguments_are_tested_as_the_ldl_twin_tests_them(qps):
    """Every bad input gives the status and the text of qps_create_csc_shared_batch; valid input (l > u in one column included: neither entry point looks at the
    order of the bounds) reaches the device test, so everything is validated before a device is needed."""
    from quadraticprogramsolver_amd import _lib
    L = _lib.lib()
    ok = _problem()
    count, n, m = ok["count"], ok["n"], ok["m"]
    Pcp, Pri, Pnz = ok["P"]
    bad_ptr = Pcp.copy(); bad_ptr[2] = bad_ptr[1] - 1                      # colptr not monotone
    bad_row = Pri.copy(); bad_row[0] = n + 3                              # row index out of range
    qnan = ok["q"].copy(); qnan[1, 2] = np.nan
    lnan = ok["l"].copy(); lnan[count - 1, 0] = np.nan
    empty = (np.zeros(n + 1, dtype=np.int64), np.zeros(1, dtype=np.int64), np.zeros(1))
    bad = [("null out", dict(), dict(out=False), BAD_ARGUMENT), ("count 0", dict(count=0), {}, BAD_DIMENSION), ("count 65536", dict(count=65536), {}, BAD_DIMENSION),
           ("n 0", dict(n=0), {}, BAD_DIMENSION), ("m -1", dict(m=-1), {}, BAD_DIMENSION), ("null q", dict(q=None), {}, BAD_ARGUMENT),
           ("index base", dict(), dict(base=2), BAD_ARGUMENT), ("dtype", dict(), dict(dtype=7), BAD_ARGUMENT),
           ("colptr", dict(P=(bad_ptr, Pri, Pnz)), {}, None), ("rowval", dict(P=(Pcp, bad_row, Pnz)), {}, None),
           ("NaN in q", dict(q=qnan), {}, NOT_FINITE), ("NaN in l", dict(l=lnan), {}, NOT_FINITE),
           ("m 0", dict(m=0, A=empty, l=None, u=None), {}, UNSUPPORTED),
           # the order: a bad count is reported ahead of a bad n, a bad n ahead of a NaN
           ("count before n", dict(count=0, n=0), {}, BAD_DIMENSION), ("n before NaN", dict(n=-3, q=qnan), {}, BAD_DIMENSION)]
    for tag, change, kw, status in bad:
        a = dict(ok, **change)
        twin, cg = _create(L, TWIN, a, **kw), _create(L, NAME, a, **kw)
        assert cg == twin and cg[0] != 0 and (status is None or cg[0] == status), (tag, cg, twin)
    lu = ok["l"].copy(); lu[1, 0] = 5.0                                    # l > u in column 1
    here = NO_DEVICE if L.qps_device_count() == 0 else 0
    for a in (ok, dict(ok, l=lu)):
        assert _create(L, NAME, a)[0] == here and _create(L, TWIN, a)[0] == here
    if L.qps_device_count() == 0:
        P, A, Q, Lo, U = random_family(3)
        with pytest.raises(qps.QpsError) as e:
            qps.QuadraticProgramCgSharedBatch(P, A, Q, Lo, U)
        assert e.value.status == NO_DEVICE


def test_no_ldl_limit_is_read(qps, monkeypatch):
    """The pattern the GPU test gives both handles: the level-scheduled plugin refuses it at creation, the CG entry point has no analysis to refuse it."""
    from quadraticprogramsolver_amd import _lib
    monkeypatch.setenv("QPS_LDL_MAX_TAIL", "64")
    monkeypatch.setenv("QPS_LDL_MAX_LEVELS", "1")
    P, A, Q, L, U = random_family(COUNT)
    with pytest.raises(qps.QpsError) as e:
        qps.QuadraticProgramSparseSharedBatch(P, A, Q, L, U)
    assert e.value.status == UNSUPPORTED
    if _lib.lib().qps_device_count() == 0:
        with pytest.raises(qps.QpsError) as e:
            qps.QuadraticProgramCgSharedBatch(P, A, Q, L, U)
        assert e.value.status == NO_DEVICE


# ---- guards on the cases, with the numpy oracle --------------------------------------------------------------------------------------------------------------
_RUNS = {}


def oracle_run(np_oracle, name, b):
    """Column b of a family to eps = 1e-6 with LinOpCg at the tight inner tolerance: flag, iterations, the largest CG count of one solve, and per check the two
    deciding ratios -- max(resPrim / epsPrim, resDual / epsDual) for convPrimDual, max(|x - xp|, |z - zp|) / epsAdmm for convAdmm."""
    if (name, b) in _RUNS:
        return _RUNS[(name, b)]
    P, A, Q, L, U = cases.family(name)
    Pd, Ad = np.asarray(sp.csc_matrix(P).todense()), np.asarray(sp.csc_matrix(A).todense())
    eps, trace, per_solve = 1e-6, [], []

    def sol(tu, vXX, vZZ, vX, mP, vQ, mA, vZ, vY, *rest):
        trace.append((vX.copy(), vZ.copy(), vY.copy()))                    # the state after iteration len(trace) - 1
        before = tu[2]["cg_iterations"]
        np_oracle.LinOpCg(tu, vXX, vZZ, vX, mP, vQ, mA, vZ, vY, *rest, ϵPcg=EPS_PCG_TIGHT, numItrPcg=ITR_PCG_TIGHT)
        per_solve.append(tu[2]["cg_iterations"] - before)

    x, info = np.zeros(Pd.shape[0]), {}
    flag = np_oracle.SolveQuadraticProgramRefLoop(x, Pd, Q[b], Ad, L[b], U[b], np_oracle.LinOpCgInit, sol, ρ=RHO[name], ϵAbs=eps, ϵRel=eps, info=info)
    trace.append((x.copy(), info["z"], info["y"]))
    ratios = []
    for ii in range(25, info["iterations"] + 1, 25):
        (xx, zz, yy), (xp, zp, _) = trace[ii], trace[ii - 1]
        Ax, Px, Aty = Ad @ xx, Pd @ xx, Ad.T @ yy
        ninf = lambda v: float(np.max(np.abs(v)))
        eP = eps + eps * max(ninf(Ax), ninf(zz))
        eD = eps + eps * max(ninf(Px), ninf(Aty), ninf(Q[b]))
        with np.errstate(invalid="ignore"):
            ratios.append((ii, max(ninf(Ax - zz) / eP, ninf(Px + Q[b] + Aty) / eD), max(ninf(xx - xp), ninf(zz - zp)) / (eps * 1e-2)))
    _RUNS[(name, b)] = dict(flag=int(flag), iterations=info["iterations"], max_cg=max(per_solve), mean_cg=sum(per_solve) / len(per_solve), ratios=ratios)
    return _RUNS[(name, b)]


@pytest.mark.parametrize("name", ["random", "banded"])
def test_family_guards_cg_counts_and_decision_margins(np_oracle, name):
    runs = [oracle_run(np_oracle, name, b) for b in range(COUNT)]
    its, flags = [r["iterations"] for r in runs], [r["flag"] for r in runs]
    nearest = min(abs(q - 1.0) for r in runs for _, a, c in r["ratios"] for q in (a, c) if not math.isnan(q))
    print(f"{name}: iterations {its}, flags {flags}, CG iterations per solve: mean {np.mean([r['mean_cg'] for r in runs]):.1f}, largest {max(r['max_cg'] for r in runs)}; "
          f"nearest deciding ratio {nearest:.4f} from 1")
    assert max(r["max_cg"] for r in runs) < ITR_PCG_TIGHT                   # the cap is no part of any compared solve
    assert nearest >= MARGIN
    assert len(set(its)) > 1 and max(its) < 5000
    if name == "random":
        assert its == RANDOM_FAMILY_ORACLE_ITERATIONS and set(flags) == {3}
    else:
        assert set(flags) == {2, 3} and 50 <= min(its) and max(its) <= 300
    # the last check decided as the flag says
    for r in runs:
        _, a, c = r["ratios"][-1]
        assert (c <= 1.0) if r["flag"] == 2 else (a < 1.0 and not c <= 1.0), r


def test_family_rho_case_guards_its_switches():
    """random20-f5 of tests/family_rho_cases.py, which the GPU test runs on both handles: no quotient rhorho / rho of any check is within 1 % of fctrRho or 1 / fctrRho."""
    f = frc.CASES["random20-f5"]["fctrRho"]
    run = frc.case_run("random20-f5", "reduced")
    assert [s[0] for s in run["switches"]] == frc.CASES["random20-f5"]["switches"]
    for ii, q in run["quotients"]:
        assert abs(q / f - 1.0) >= MARGIN and abs(q * f - 1.0) >= MARGIN, (ii, q)


def test_polish_family_has_no_row_whose_sign_is_noise(np_oracle):
    """What test_polish_matches_the_ldl_handle relies on: at the stopping iterate every free row has y = 0 exactly and every equality row a y far from 0."""
    P, A, Q, L, U = cases.polish_family(COUNT)
    Pd, Ad = np.asarray(P.todense()), np.asarray(A.todense())
    assert np.array_equal(L[:, :5], U[:, :5]) and np.all(np.isinf(L[:, 5:])) and np.all(np.isinf(U[:, 5:]))
    for b in (0, 3, 17):
        x, info = np.zeros(Pd.shape[0]), {}
        np_oracle.SolveQuadraticProgramRefLoop(x, Pd, Q[b], Ad, L[b], U[b], np_oracle.RedCholInit, np_oracle.RedChol, ρ=1.0, info=info)
        assert not info["y"][5:].any() and np.abs(info["y"][:5]).min() > 1e-4, b


# ---- the dispatch of k_cg_panel.hip restated -------------------------------------------------------------------------------------------------------------------
def test_dispatch_reaches_every_strip_count_and_a_ragged_last_workgroup():
    P, A = random_family(1)[:2]
    Pb, Ab = banded_family(1)[:2]
    n, m, nb, mb = P.shape[0], A.shape[0], Pb.shape[0], Ab.shape[0]
    assert (n, m, nb, mb) == (100, 50, 70, 139)
    pn, an = sp.csc_matrix(P).nnz, sp.csc_matrix(A).nnz
    print(f"random: mean row of P {pn / n:.2f}, of A {an / m:.2f}, of A' {an / n:.2f}; banded: {Pb.nnz / nb:.2f}, {Ab.nnz / mb:.2f}, {Ab.nnz / nb:.2f}")
    assert cases.launch_sprs(P, A) == dict(rhs=4, av=4, post=4, op=16)
    assert cases.launch_sprs(Pb, Ab) == dict(rhs=1, av=1, post=1, op=1)
    assert 8.0 < an / n < 8.1                                              # just above the cut between one strip and four
    # rows per workgroup 16 / 4 / 1; a last workgroup with fewer valid rows than it holds in the two bands where a workgroup holds more than one row
    assert [cases.geometry(1000, s)[0] for s in (1, 4, 16)] == [16, 4, 1]
    assert cases.last_group_valid_rows(mb, 1) == 11 and cases.last_group_valid_rows(nb, 1) == 6        # banded: A u / post over 139 rows, the operator over 70
    assert cases.last_group_valid_rows(m, 4) == 2                                                      # random: A u / post over 50 rows
    assert cases.last_group_valid_rows(n, 16) == 1                                                     # 16 strips: one row per workgroup, never ragged
    # partials: one workgroup per row group up to 2048 (operator) / 256 (vector kernels) groups, then several rounds per workgroup
    assert cases.geometry(n, 16) == (1, 1, 100) and cases.geometry(nb, 1) == (16, 1, 5) and cases.geometry(n) == (16, 1, 7) and cases.geometry(nb) == (16, 1, 5)
    assert cases.geometry(16 * 2048, 1) == (16, 1, 2048) and cases.geometry(16 * 256) == (16, 1, 256)
    # test_more_row_groups_than_workgroups: 2063 row groups; the operator takes two rounds per workgroup and its last workgroup one, the vector kernels nine
    # and their last workgroup two
    assert cases.geometry(cases.LONG_N, 1) == (16, 2, 1032) and 1032 * 2 - 2063 == 1
    assert cases.geometry(cases.LONG_N) == (16, 9, 230) and 230 * 9 - 2063 == 7
