"""CPU-only checks of the family-wide adaptive rho of the shared-matrix batches (qps_set_shared_adaptive_rho): the symbol is declared, exported and bound in
header, library, ctypes and Julia; a NULL handle and a bad mode are refused without a device; at count = 1 the numpy restatement of tests/family_rho_cases.py --
the reference of the GPU tests -- is the reference loop with adptΡ = true; and every row of the case table passes its guard: both linear-system forms take the
same decisions, no decision of the rule sits on a rounding edge, and the two forms agree in the switched rho to what the GPU bound of the row allows.  The
proposal the library itself computes (family_rho_proposal of csrc/shared_family_rules.h, through the host-test shim) equals that restatement to the last bit."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from family_rho_cases import CASES, EPS, NUM_ITR_CONV, RHO, FamilyRestatement, case_run, family_proposal
from host_shim import rules
from oracle.qps_oracle_np import RedChol, RedCholInit, SolveQuadraticProgramRefLoop
from shared_batch_cases import shared_family

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "qps_set_shared_adaptive_rho"
BAD_ARGUMENT = 1


def test_symbol_is_declared_exported_and_bound(qps):
    from quadraticprogramsolver_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qps.h")).read(), flags=re.S)
    assert re.search(r"\bint32_t\s+%s\s*\(\s*qps_handle\s+\w+\s*,\s*int32_t\s+\w+\s*\)" % NAME, header), f"{NAME} is not declared in include/qps.h"
    assert NAME in _lib.EXPORTED_SYMBOLS
    assert hasattr(C.CDLL(_lib.LIB_PATH), NAME), f"{NAME} is not exported by the library"
    fn = getattr(_lib.lib(), NAME)
    assert fn.restype is C.c_int32 and list(fn.argtypes) == [C.c_void_p, C.c_int32]
    jl = re.sub(r"#[^\n]*", "", open(os.path.join(ROOT, "julia", "QuadraticProgramSolverHIP.jl"), encoding="utf-8").read())
    assert re.search(r"ccall\(\(:%s,\s*LIBQPS\),\s*Int32,\s*\(Ptr\{Cvoid\},\s*Int32\)" % NAME, jl), f"{NAME} has no ccall in the Julia binding"
    assert hasattr(qps.QuadraticProgramSharedBatch, "set_adaptive_rho")
    assert qps.QuadraticProgramSparseSharedBatch.set_adaptive_rho is qps.QuadraticProgramSharedBatch.set_adaptive_rho


def test_null_handle_and_bad_mode_are_refused_without_a_device(qps):
    from quadraticprogramsolver_amd import _lib
    L = _lib.lib()
    for mode in (0, 1, 2, -1):
        assert L.qps_set_shared_adaptive_rho(None, mode) == BAD_ARGUMENT
    assert b"NULL" in L.qps_last_error(None)


def test_proposal_picks_the_worst_running_columns():
    """Ties go to the lowest column, a NaN quotient never wins against a number, the four norms may come from two columns, no running column leaves rhorho alone,
    and the clamp is the reference's."""
    norms = {0: (1.0, 1.0, 10.0, 10.0), 1: (4.0, 0.5, 10.0, 10.0), 2: (4.0, 2.0, 10.0, 5.0), 3: (np.nan, np.nan, 1.0, 1.0)}
    # bp = 1 (0.4, tie with 2 -> lowest), bd = 2 (0.4): rho sqrt(4 * 5 / (2 * 10)) = rho
    assert family_proposal(norms, [0, 1, 2, 3], 0.1, 7.0) == 0.1
    assert family_proposal(norms, [2, 3], 0.1, 7.0) == 0.1 * np.sqrt((4.0 * 5.0) / (2.0 * 10.0))
    assert family_proposal(norms, [0], 0.1, 7.0) == 0.1                              # one column: its own four norms
    assert np.isnan(family_proposal(norms, [3], 0.1, 7.0))                           # all NaN: a NaN proposal, which never passes the switch test
    assert family_proposal(norms, [], 0.1, 7.0) == 7.0
    assert family_proposal({0: (1.0, 1e-20, 1.0, 1.0)}, [0], 1.0, 1.0) == 1e6 and family_proposal({0: (1e-20, 1.0, 1.0, 1.0)}, [0], 1.0, 1.0) == 1e-3


NAN = float("nan")
# (name, norms per column as (normResPrim, normResDual, maxNormPrim, maxNormDual), running columns, rho, rhorho)
PROPOSAL_INPUTS = [
    ("three columns, the norms from two of them", [(1.0, 1.0, 10.0, 10.0), (3.0, 0.5, 10.0, 10.0), (0.7, 2.0, 10.0, 5.0)], [0, 1, 2], 0.1, 7.0),
    ("a tie: the lowest index wins", [(1.0, 1.0, 10.0, 10.0), (4.0, 0.5, 10.0, 10.0), (4.0, 2.0, 10.0, 5.0), (8.0, 3.0, 20.0, 7.5)], [0, 1, 2, 3], 0.1, 7.0),
    ("a NaN quotient loses to a number, first or last", [(NAN, NAN, 1.0, 1.0), (0.3, 0.2, 7.0, 3.0), (NAN, 0.1, 1.0, 3.0)], [0, 1, 2], 0.25, 7.0),
    ("all quotients NaN", [(NAN, NAN, 1.0, 1.0), (NAN, NAN, 2.0, 2.0)], [0, 1], 0.1, 7.0),
    ("one running column of three", [(1.0, 1.0, 10.0, 10.0), (0.3, 0.011, 7.0, 3.0), (9.0, 9.0, 1.0, 1.0)], [1], 0.1, 7.0),
    ("no running column: rhorho comes back", [(1.0, 1.0, 10.0, 10.0), (0.3, 0.011, 7.0, 3.0)], [], 0.1, 7.0),
    ("clamped at 1e6", [(1.0, 1e-20, 1.0, 1.0)], [0], 1.0, 1.0),
    ("clamped at 1e-3", [(1e-20, 1.0, 1.0, 1.0)], [0], 1.0, 1.0),
    ("a zero dual residual: the denominator is 0", [(0.5, 0.0, 2.0, 3.0), (0.25, 0.0, 2.0, 3.0)], [0, 1], 0.1, 7.0),
    ("zero over zero", [(0.0, 0.0, 2.0, 3.0)], [0], 0.1, 7.0),
    ("a zero maximum norm: an infinite quotient wins", [(0.5, 0.5, 0.0, 3.0), (0.25, 0.75, 2.0, 3.0)], [0, 1], 0.1, 7.0),
]


@pytest.mark.parametrize("name,norms,running,rho,rhorho", PROPOSAL_INPUTS, ids=[c[0] for c in PROPOSAL_INPUTS])
def test_the_library_proposal_is_the_restatement_to_the_last_bit(name, norms, running, rho, rhorho):
    """family_rho_proposal as the solvers call it -- 8 doubles per column, one active word per column -- against family_proposal: the same double, or NaN on both
    sides (a NaN carries no value to compare).  The expected values of the plain cases are written out as well, so the two cannot be wrong together there."""
    count = len(norms)
    res = np.full(8 * count, -777.0)                             # slots 4..7 of a column are not the rule's business
    for b, four in enumerate(norms):
        res[8 * b:8 * b + 4] = four
    act = np.zeros(count, dtype=np.int32); act[running] = 1
    got = rules().lt_family_rho_proposal(res.ctypes.data_as(C.POINTER(C.c_double)), act.ctypes.data_as(C.POINTER(C.c_int)), count, rho, rhorho)
    want = family_proposal(dict(enumerate(norms)), running, rho, rhorho)
    print(f"{name}: library {got!r}, restatement {want!r}")
    assert (math.isnan(got) and math.isnan(want)) or got == want
    by_hand = {"three columns, the norms from two of them": 0.1 * math.sqrt((3.0 * 5.0) / (2.0 * 10.0)), "a tie: the lowest index wins": 0.1,
               "no running column: rhorho comes back": 7.0, "clamped at 1e6": 1e6, "clamped at 1e-3": 1e-3, "a zero dual residual: the denominator is 0": 1e6}
    if name in by_hand:
        assert got == by_hand[name]
    if name in ("all quotients NaN", "zero over zero"):
        assert math.isnan(got)


@pytest.mark.parametrize("b", [0, 1, 3])
def test_count_one_is_the_reference_loop_with_adaptive_rho(b):
    """With one column the rule is SolveQuadraticProgram.jl:92-96 and :47 expression for expression: against SolveQuadraticProgramRefLoop(..., adptΡ=True) with the
    reduced Cholesky pair -- same switches, flag and stopping iteration, x to 1e-12 (measured <= 6e-16 on these columns)."""
    P, A, Q, L, U = shared_family(96, 160, 4)
    r = FamilyRestatement(P, A, form="reduced").solve(Q[b], L[b], U[b], fctrRho=5.0)
    col = r["columns"][0]
    x, info = np.zeros(96), {}
    flag = SolveQuadraticProgramRefLoop(x, P, Q[b], A, L[b], U[b], RedCholInit, RedChol, numIterations=5000, ϵAbs=EPS, ϵRel=EPS, ρ=RHO, adptΡ=True, fctrΡ=5,
                                        numItrConv=NUM_ITR_CONV, info=info)
    dev = np.abs(col["x"] - x).max()
    print(f"column {b}: flag {col['convFlag']}/{int(flag)} iterations {col['iterations']}/{info['iterations']} switches {r['switches']} max|dx| {dev:.2e}")
    assert col["convFlag"] == int(flag) and col["iterations"] == info["iterations"]
    assert col["numRefactor"] == info["n_refactor"] == len(r["switches"]) and col["numRefactor"] >= 1
    # the new rho is rho sqrt of a quotient of residual norms: differences of O(1) vectors that have shrunk to 1e-3 .. 1e-5 by the first checks, so the rounding of
    # two summation orders (1e-16) comes back 1e3 .. 1e5 times larger; measured 1e-12 here
    print(f"column {b}: rhoFinal {col['rhoFinal']!r} against {info['rho_final']!r}")
    assert abs(col["rhoFinal"] - info["rho_final"]) <= 1e-10 * info["rho_final"]
    assert dev <= 1e-12


@pytest.mark.parametrize("name", list(CASES))
def test_case_guard(name):
    """A GPU test must not hide a decision that sits on a rounding edge: the reduced and the KKT form agree in flags, stopping iterations and switch iterations,
    and at every check rhorho / rho stays at least 2 % away from fctrRho and from 1 / fctrRho.  The figures are those of the case table."""
    c, f = CASES[name], CASES[name]["fctrRho"]
    red, kkt = case_run(name, "reduced"), case_run(name, "kkt")
    for r in (red, kkt):
        assert [s[0] for s in r["switches"]] == c["switches"]
        assert [k["iterations"] for k in r["columns"]] == c["iterations"]
        assert [k["convFlag"] for k in r["columns"]] == c["flags"]
        assert [k["numRefactor"] for k in r["columns"]] == [sum(1 for s in c["switches"] if s <= it) for it in c["iterations"]]
        edge = min(min(abs(q / f - 1.0), abs(q * f - 1.0)) for _, q in r["quotients"])
        print(f"{name}: switches {[(s[0], s[2]) for s in r['switches']]}, closest quotient to fctrRho or 1 / fctrRho: {edge:.3f} relative")
        assert edge >= 0.02
    assert [i for i, _ in red["quotients"]] == [i for i, _ in kkt["quotients"]]
    # the reference's own error in the switched rho: a late proposal divides residual norms that have shrunk by orders of magnitude, so the two exact forms drift
    # apart.  A row is held to the spread it records (the GPU bound is ten times that), a row that records none to a tenth of the GPU bound of 1e-10.
    spread = [abs(a - b) / b for (_, _, a), (_, _, b) in zip(red["switches"], kkt["switches"])]
    print("new rho, reduced against kkt, relative:", [f"{v:.1e}" for v in spread])
    assert max(spread) <= c.get("rho_spread", 1e-11)
    assert len(c["switches"]) >= 1


def test_fixed_rho_restatement_is_the_rho_scale_restatement():
    """adaptive=False is the fixed-rho loop the existing tests use (tests/rho_scale_cases.py), column by column."""
    from rho_scale_cases import Restatement
    P, A, Q, L, U = shared_family(96, 160, 4)
    r = FamilyRestatement(P, A, form="reduced").solve(Q, L, U, adaptive=False, numIterations=100, epsAbs=0.0, epsRel=0.0)
    one = Restatement(P, A, np.ones(160), form="reduced", rho=RHO)
    for b in range(4):
        ref = one.solve(Q[b], L[b], U[b], numIterations=100, epsAbs=0.0, epsRel=0.0)
        assert np.abs(r["columns"][b]["x"] - ref["x"]).max() <= 1e-12 * max(1.0, np.abs(ref["x"]).max())
        assert r["columns"][b]["numRefactor"] == 0 and r["columns"][b]["rhoFinal"] == RHO
    assert r["switches"] == []
