"""CPU-only checks of the opt-in infeasibility certificates of the shared-matrix batches (qps_set_shared_infeasibility, qps_get_shared_certificate): both symbols
and the two new flags are declared, exported and bound in header, library, ctypes, Python and Julia; a NULL handle and bad values are refused without a device;
the numpy restatement of tests/infeasibility_cases.py -- the reference of the GPU tests -- is FamilyRestatement with the option off; every row of the case table
is reproduced by both linear-system forms; every builder's proof of infeasibility holds; and no decision of any case sits on a rounding edge."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from family_rho_cases import FamilyRestatement
from family_rho_cases import case_data as family_case_data
from infeasibility_cases import (BUILDERS, CASES, DUAL_INFEASIBLE, EPS_INF, MARGIN, PRIM_INFEASIBLE, InfeasibilityRestatement, case_data, case_run, certificate_holds, dense_primal,
                                 farkas_primal, project_dy, robust)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARGUMENT = 1


def test_symbols_are_declared_exported_and_bound(qps):
    from quadraticprogramsolver_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qps.h")).read(), flags=re.S)
    assert re.search(r"\bint32_t\s+qps_set_shared_infeasibility\s*\(\s*qps_handle\s+\w+\s*,\s*double\s+\w+\s*,\s*double\s+\w+\s*\)\s*;", header)
    assert re.search(r"\bint32_t\s+qps_get_shared_certificate\s*\(\s*qps_handle\s+\w+\s*,\s*double\s*\*\s*\w+\s*,\s*double\s*\*\s*\w+\s*\)\s*;", header)
    assert re.search(r"\bQPS_CONV_PRIMAL_INFEASIBLE\s*=\s*4\b", header) and re.search(r"\bQPS_CONV_DUAL_INFEASIBLE\s*=\s*5\b", header)
    jl = re.sub(r"#[^\n]*", "", open(os.path.join(ROOT, "julia", "QuadraticProgramSolverHIP.jl"), encoding="utf-8").read())
    assert re.search(r"ccall\(\(:qps_set_shared_infeasibility,\s*LIBQPS\),\s*Int32,\s*\(Ptr\{Cvoid\},\s*Float64,\s*Float64\)", jl)
    assert re.search(r"ccall\(\(:qps_get_shared_certificate,\s*LIBQPS\),\s*Int32,\s*\(Ptr\{Cvoid\},\s*Ptr\{Float64\},\s*Ptr\{Float64\}\)", jl)
    assert re.search(r"convPrimInfeasible\s*=\s*4\b", jl) and re.search(r"convDualInfeasible\s*=\s*5\b", jl)
    dp = C.POINTER(C.c_double)
    for name, args in (("qps_set_shared_infeasibility", [C.c_void_p, C.c_double, C.c_double]), ("qps_get_shared_certificate", [C.c_void_p, dp, dp])):
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(C.CDLL(_lib.LIB_PATH), name), f"{name} is not exported by the library"
        fn = getattr(_lib.lib(), name)
        assert fn.restype is C.c_int32 and list(fn.argtypes) == args
    assert int(qps.ConvergenceFlag.convPrimInfeasible) == PRIM_INFEASIBLE and int(qps.ConvergenceFlag.convDualInfeasible) == DUAL_INFEASIBLE
    for method in ("set_infeasibility", "certificate"):
        assert getattr(qps.QuadraticProgramSparseSharedBatch, method) is getattr(qps.QuadraticProgramSharedBatch, method)


def test_null_handle_and_bad_values_are_refused_without_a_device(qps):
    from quadraticprogramsolver_amd import _lib
    L = _lib.lib()
    for ep, ed in ((0.0, 0.0), (1e-4, 1e-4), (-1.0, 1e-4), (1e-4, float("nan")), (float("inf"), 0.0)):
        assert L.qps_set_shared_infeasibility(None, ep, ed) == BAD_ARGUMENT
    assert b"NULL" in L.qps_last_error(None)
    z = np.zeros(4)
    ptr = z.ctypes.data_as(C.POINTER(C.c_double))
    assert L.qps_get_shared_certificate(None, ptr, ptr) == BAD_ARGUMENT and L.qps_get_shared_certificate(None, None, None) == BAD_ARGUMENT


def test_python_values(qps):
    """None / False / 0 / a number are marshalled as doubles and reach the library (which refuses the probe's NULL handle); anything else is a Python error."""
    class Probe(qps.QuadraticProgramSharedBatch):          # no handle: only the argument handling runs
        def __init__(self):
            self._h = None

        def close(self):
            pass

    for args in ((), (None, None), (False, 1e-3), (0, 0), (2e-4,)):
        with pytest.raises(qps.QpsError) as e:
            Probe().set_infeasibility(*args)
        assert e.value.status == BAD_ARGUMENT
    with pytest.raises((TypeError, ValueError)):
        Probe().set_infeasibility("yes")


@pytest.mark.parametrize("form", ["reduced", "kkt"])
def test_with_the_option_off_it_is_the_family_restatement(form):
    """shared96-f5 of tests/family_rho_cases.py, under the family rule and at a fixed rho: every column, every info field and the switches, bit for bit."""
    P, A, Q, L, U, s, f = family_case_data("shared96-f5")
    for adaptive in (True, False):
        kw = dict(fctrRho=f, adaptive=adaptive, numIterations=300)
        a = InfeasibilityRestatement(P, A, 0, s, form=form).solve(Q, L, U, **kw)
        b = FamilyRestatement(P, A, s, form=form).solve(Q, L, U, **kw)
        assert a["switches"] == b["switches"] and a["quotients"] == b["quotients"]
        for ca, cb in zip(a["columns"], b["columns"]):
            assert all(np.array_equal(ca[k], cb[k]) for k in ("x", "z", "y"))
            assert all(ca[k] == cb[k] for k in ("convFlag", "iterations", "numRefactor", "rhoFinal", "rhoProposed", "resPrim", "resDual"))
            assert not ca["dy"].any() and not ca["dx"].any()
        assert all(e["primal"] is None and e["dual"] is None for e in a["trace"])


def test_projection_and_validity_helpers():
    l, u = np.array([-np.inf, -np.inf, 0.0, 0.0]), np.array([np.inf, 1.0, np.inf, 1.0])
    assert np.array_equal(project_dy(np.array([3.0, -2.0, 2.0, -2.0]), l, u), [0.0, 0.0, 0.0, -2.0])
    assert np.array_equal(project_dy(np.array([-3.0, 2.0, -2.0, 2.0]), l, u), [0.0, 2.0, -2.0, 2.0])
    assert np.isnan(project_dy(np.array([0.0, np.nan, np.nan, np.nan]), l, u)[1:]).all()
    assert robust([(1.5, "above"), (0.5, "below")]) and robust([(1.001, "above"), (1.5, "below")]) and not robust([(1.001, "above"), (0.5, "below")])
    P, A, Q, L, U = case_data("known-primal")
    dy = np.array([-2.0, 2.0, 0.0])
    assert certificate_holds(P, A, Q[1], L[1], U[1], dy, np.zeros(2), PRIM_INFEASIBLE, 1e-4, 1e-4)
    assert not certificate_holds(P, A, Q[0], L[0], U[0], dy, np.zeros(2), PRIM_INFEASIBLE, 1e-4, 1e-4)        # column 0 is feasible: the same vector proves nothing
    assert not certificate_holds(P, A, Q[1], L[1], U[1], -dy, np.zeros(2), PRIM_INFEASIBLE, 1e-4, 1e-4)       # outside the cone
    assert not certificate_holds(P, A, Q[1], L[1], U[1], np.array([np.nan, 2.0, 0.0]), np.zeros(2), PRIM_INFEASIBLE, 1e-4, 1e-4)
    P, A, Q, L, U = case_data("known-dual")
    assert certificate_holds(P, A, Q[1], L[1], U[1], np.zeros(2), np.array([3.0, 0.0]), DUAL_INFEASIBLE, 1e-4, 1e-4)
    assert not certificate_holds(P, A, Q[0], L[0], U[0], np.zeros(2), np.array([3.0, 0.0]), DUAL_INFEASIBLE, 1e-4, 1e-4)
    assert not certificate_holds(P, A, Q[1], L[1], U[1], np.zeros(2), np.array([0.0, 3.0]), DUAL_INFEASIBLE, 1e-4, 1e-4)


def test_every_builder_asserts_its_proof():
    """The builders raise when their exact proof fails; c = 0.5 is not enough for the wide bounds of column 4, which is why the assert is there."""
    for name in BUILDERS:
        assert len(BUILDERS[name](*next((c.get("args", ()) for c in CASES.values() if c["builder"] == name), ()))) == 5
    with pytest.raises(AssertionError):
        dense_primal(6, {4: 0.5})
    for name, c in CASES.items():
        if c["builder"] in ("dense_primal", "sparse_primal") and not c.get("scrambled"):
            P, A, Q, L, U = case_data(name)
            for b, flag in enumerate(c["flags"]):
                if flag == PRIM_INFEASIBLE:
                    assert np.all(np.isfinite(L[b])) and np.all(L[b] <= U[b])          # infeasible through the rows together, not through a crossed pair of bounds


@pytest.mark.parametrize("name", list(CASES))
def test_case_table_and_rounding_guard(name):
    """Both forms reproduce the row, with and without the option, and a GPU test cannot hide a decision on a rounding edge.  At every check of the case, for every
    column examined at it, each of the four tests -- CheckConvergence's residual pair and stall pair, the primal and the dual certificate test -- is decided with
    the project's 2 % margin: all of its comparisons pass by it, or at least one fails by it (a comparison that sits on its threshold decides nothing while
    another fails clearly).  The check before a certificate fires is one of those checks, so there the test fails by the margin; and under the family rule every
    proposal is 2 % clear of the fctrRho band's edges.  A feasible column never receives flag 4 or 5."""
    c = CASES[name]
    figures = []
    for form in ("reduced", "kkt"):
        run = case_run(name, form)
        assert [k["convFlag"] for k in run["columns"]] == c["flags"], form
        assert [k["iterations"] for k in run["columns"]] == c["iterations"], form
        assert [s[0] for s in run["switches"]] == c.get("switches", []), form
        closest = np.inf
        for e in run["trace"]:
            for test in ("primdual", "admm", "primal", "dual"):
                if e[test] is not None:
                    assert robust(e[test]), (name, form, e["ii"], e["b"], test, e[test])
                    closest = min(closest, min(abs(float(q) - 1.0) for q, _ in e[test] if not np.isnan(q)))
            assert (e["primal"] is not None) == (e["flag"] in (1, PRIM_INFEASIBLE, DUAL_INFEASIBLE)), "a column CheckConvergence decided is not examined"
        f = c["solve"].get("fctrRho")
        for _, q in run["quotients"]:
            assert abs(q / f - 1.0) > MARGIN and abs(q * f - 1.0) > MARGIN, (name, form, q)
        fired = [e for e in run["trace"] if e["flag"] in (PRIM_INFEASIBLE, DUAL_INFEASIBLE)]
        assert sorted(e["b"] for e in fired) == [b for b, fl in enumerate(c["flags"]) if fl in (PRIM_INFEASIBLE, DUAL_INFEASIBLE)]
        for e in fired:
            before = [p for p in run["trace"] if p["b"] == e["b"] and p["ii"] == e["ii"] - 25]
            if before:                                      # (a certificate at the first check has no check before it)
                t = "primal" if e["flag"] == PRIM_INFEASIBLE else "dual"
                assert any((q < 1.0 - MARGIN) if side == "above" else (q > 1.0 + MARGIN) for q, side in before[0][t]), (name, form, before[0][t])
        print(f"{name} {form}: smallest distance of a compared quotient from 1 over all checks (robust decisions only): {closest:.3e}")
        figures.append(closest)
        if "off" in c:
            off = case_run(name, form, on=False)
            assert [k["convFlag"] for k in off["columns"]] == c["off"]["flags"] and [k["iterations"] for k in off["columns"]] == c["off"]["iterations"], form
            assert [s[0] for s in off["switches"]] == c["off"].get("switches", []), form
            for e in off["trace"]:
                assert robust(e["primdual"]) and robust(e["admm"]), (name, form, "off", e["ii"], e["b"])
            for _, q in off["quotients"]:
                assert abs(q / f - 1.0) > MARGIN and abs(q * f - 1.0) > MARGIN, (name, form, "off", q)
    assert abs(figures[0] - figures[1]) <= 1e-5 * max(1.0, figures[0])


@pytest.mark.parametrize("name", list(CASES))
def test_certificates_of_the_restatement_are_valid_and_feasible_columns_get_none(name):
    c = CASES[name]
    P, A, Q, L, U = case_data(name)
    run = case_run(name)
    for b, col in enumerate(run["columns"]):
        assert certificate_holds(P, A, Q[b], L[b], U[b], col["dy"], col["dx"], col["convFlag"], c.get("eps_p", EPS_INF), c.get("eps_d", EPS_INF)), (name, b)
        if col["convFlag"] not in (PRIM_INFEASIBLE, DUAL_INFEASIBLE):
            assert not col["dy"].any() and not col["dx"].any()
    if c["builder"] in ("dense_primal", "sparse_primal") and not c.get("scrambled"):
        for b, col in enumerate(run["columns"]):
            S, At = farkas_primal(A, L[b], U[b], col["dy"]) if col["convFlag"] == PRIM_INFEASIBLE else (-1.0, 0.0)
            assert S < 0 and At <= c.get("eps_p", EPS_INF) * np.abs(col["dy"]).max()          # the returned dyh is itself an approximate Farkas proof
