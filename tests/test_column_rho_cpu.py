"""CPU-only checks of the per-column adaptive rho of the CG shared-matrix batch (qps_set_shared_column_rho): the symbol is declared, exported and bound in
header, library, ctypes and Julia; a NULL handle and a bad argument are refused without a device; and the numpy restatement of tests/column_rho_cases.py -- the
yardstick of the GPU tests beside the C oracle -- takes, column by column, the decisions of the C oracle's matrix-free CG and of its sparse L D L' with adptRho.
The guard re-derives which columns a GPU test may compare (decisions clear of their thresholds) and re-measures the spread between the oracle's two
linear-system paths that the GPU tolerances are built from."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import column_rho_cases as crc
from cg_shared_cases import LONG_N, banded_family

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "qps_set_shared_column_rho"
BAD_ARGUMENT = 1


def rel(a, b):
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


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
    assert hasattr(qps.QuadraticProgramCgSharedBatch, "set_column_rho")
    assert qps.QuadraticProgramSparseSharedBatch.set_column_rho is qps.QuadraticProgramSharedBatch.set_column_rho is qps.QuadraticProgramCgSharedBatch.set_column_rho


def test_null_handle_is_refused_without_a_device(qps):
    from quadraticprogramsolver_amd import _lib
    L = _lib.lib()
    for on in (0, 1, 2, -1):
        assert L.qps_set_shared_column_rho(None, on) == BAD_ARGUMENT
    assert b"NULL" in L.qps_last_error(None)


def test_one_column_proposal_is_the_library_rule():
    """family_rho_proposal with a mask that holds one column -- what the driver calls per column -- is the restatement's expression to the last bit."""
    from host_shim import rules
    act = np.ones(1, dtype=np.int32)
    for norms, rho in (((0.3, 0.011, 7.0, 3.0), 0.1), ((1.0, 1e-20, 1.0, 1.0), 1.0), ((1e-20, 1.0, 1.0, 1.0), 1.0), ((0.0, 0.0, 2.0, 3.0), 0.1), ((2.5e-4, 3.5e-2, 11.0, 0.7), 37.5)):
        res = np.full(8, -777.0); res[:4] = norms
        got = rules().lt_family_rho_proposal(res.ctypes.data_as(C.POINTER(C.c_double)), act.ctypes.data_as(C.POINTER(C.c_int)), 1, rho, 7.0)
        want = crc.proposal(norms, rho)
        assert (np.isnan(got) and np.isnan(want)) or got == want, (norms, got, want)


@pytest.mark.parametrize("fixed_k", [None, crc.FIXED_K], ids=["eps1e-6", "k100"])
@pytest.mark.parametrize("name", list(crc.CASES))
def test_case_guard(c_oracle, name, fixed_k):
    """The restatement against the C oracle's matrix-free CG and sparse L D L', every column with adptRho.  On every compared column flag, iterations and
    numRefactor agree between all three; at most MAX_LEFT_OUT of 20 columns are left out; the compared columns of a case take at least two different switch
    sets; and the spread between the oracle's two paths stays inside the row of the case table the GPU tolerances come from."""
    cols = crc.case_run(name, fixed_k=fixed_k)
    red = crc.case_run(name, form="reduced", fixed_k=fixed_k)
    cg, ldl = crc.oracle_run(name, "cg", fixed_k), crc.oracle_run(name, "ldl", fixed_k)
    keep = crc.compared(cols)
    left = sorted(set(range(crc.COUNT)) - set(keep))
    print(f"{name} fixed_k={fixed_k}: left out {left}: " + ", ".join(f"column {b} switch margin {crc.switch_clearance(cols[b]):.4f} stop margin {crc.stop_clearance(cols[b]):.4f}" for b in left))
    assert len(left) <= crc.MAX_LEFT_OUT
    spread = dict(rho=0.0, x=0.0, z=0.0, y=0.0)
    for b in keep:
        k = cols[b]
        sw = [s[0] for s in k["switches"]]
        print(f"column {b}: flag {k['convFlag']} iterations {k['iterations']} switches at {sw} rhoFinal {k['rhoFinal']:.6g} switch margin "
              f"{crc.switch_clearance(k):.3f} stop margin {crc.stop_clearance(k):.3f}")
        assert [s[0] for s in red[b]["switches"]] == sw and red[b]["iterations"] == k["iterations"] and red[b]["convFlag"] == k["convFlag"], b
        for tag, (xo, io) in (("cg", cg[b]), ("ldl", ldl[b])):
            assert (io["convFlag"], io["iterations"], io["numRefactor"]) == (k["convFlag"], k["iterations"], k["numRefactor"]), (tag, b, io["convFlag"], io["iterations"], io["numRefactor"])
        (xc, ic), (xl, il) = cg[b], ldl[b]
        spread["rho"] = max(spread["rho"], abs(ic["rhoFinal"] - il["rhoFinal"]) / il["rhoFinal"])
        spread["x"] = max(spread["x"], rel(xc, xl)); spread["z"] = max(spread["z"], rel(ic["z"], il["z"])); spread["y"] = max(spread["y"], rel(ic["y"], il["y"]))
        # the restatement is a third correct path: it lies as close to the L D L' oracle as the CG oracle does, to the bound the device is held to
        tol = crc.tolerances(name, bool(fixed_k))
        fig = (abs(k["rhoFinal"] - il["rhoFinal"]) / il["rhoFinal"], rel(k["x"], xl), rel(k["z"], il["z"]), rel(k["y"], il["y"]))
        assert all(f <= t for f, t in zip(fig, tol)), (b, fig, tol)
    row = crc.CASES[name]["spread_k100" if fixed_k else "spread"]
    print(f"{name} fixed_k={fixed_k}: spread CG against L D L' over {len(keep)} columns: " + " ".join(f"{q} {v:.1e}" for q, v in spread.items()) + f"; table {row}")
    # the figures are rounding noise amplified by the loop, and the oracle's sums depend on its thread count: a row is stale when a figure leaves it by more
    # than a factor of two (below 1e-12 nothing is told apart: the bounds built from such a row are the fixed-rho floors)
    assert all(spread[q] <= max(2.0 * row[q], 1e-12) for q in spread), (spread, row)
    sets = {tuple(s[0] for s in cols[b]["switches"]) for b in keep}
    print(f"{name}: {len(sets)} different switch sets among the compared columns, final rho from {min(cols[b]['rhoFinal'] for b in keep):.3g} to "
          f"{max(cols[b]['rhoFinal'] for b in keep):.3g}")
    assert len(sets) >= 2


@pytest.mark.parametrize("name", list(crc.CASES))
def test_never_switching_setting_produces_no_switch(name):
    for fixed_k in (None, crc.FIXED_K):
        cols = crc.case_run(name, fixed_k=fixed_k, fctrRho=crc.NEVER)
        assert all(k["numRefactor"] == 0 and k["rhoFinal"] == crc.CASES[name]["rho"] for k in cols)
    fixed = crc.ColumnRestatement(*crc.case_data(name)[:2]).solve(*crc.case_data(name)[2:], rho=crc.CASES[name]["rho"], fctrRho=5.0, adaptive=False,
                                                                   numIterations=crc.FIXED_K, epsAbs=0.0, epsRel=0.0)
    for a, b in zip(fixed, crc.case_run(name, fixed_k=crc.FIXED_K, fctrRho=crc.NEVER)):
        assert np.array_equal(a["x"], b["x"]) and np.array_equal(a["y"], b["y"])


def test_fp32_case_has_enough_columns_to_compare():
    """fp32, K = 100 on the banded case: only columns whose decisions up to K are 10 % clear are compared -- and, of those, only the ones whose residual norms
    fp32 can resolve at every check that feeds a decision (fp32_resolves) -- and those are at least 10 of 20."""
    cols = crc.case_run("banded20-f5", fixed_k=crc.FIXED_K)
    clear = crc.compared(cols, switch_clear=crc.FP32_CLEAR, stop_clear=0.0, upto=crc.FIXED_K)
    keep = crc.compared_fp32(cols, crc.FIXED_K)
    print("10 % clear:", clear, "of those resolved by fp32:", keep)
    assert set(keep) <= set(clear) and len(keep) >= 10
    # what the second condition removes, and why: column 18 takes a proposal formed on a relative dual residual of 4.5e-8, below half an ulp of fp32; columns 17
    # and 19 have converged to relative residuals of 5e-9 and 1e-11 by iteration 75, where the quotient of two such norms is rounding noise in fp32
    assert len(clear) == 16 and sorted(set(clear) - set(keep)) == [17, 18, 19]


def test_long_case_switches_at_iteration_26(c_oracle):
    """banded_family(3, n=LONG_N) at rho = LONG_RHO, K = 30: the C oracle's CG switches every column at the top of iteration 26, the proposal at least 5 % clear
    of both thresholds (the size is beyond a dense restatement; after the one switch rhoFinal is the proposal of the check at 25).  The spread against the
    oracle's sparse L D L' is the row the GPU tolerances of this size come from."""
    P, A, Q, L, U = banded_family(3, n=LONG_N)
    kw = dict(rho=crc.LONG_RHO, fctrRho=5.0, adptRho=True, numIterations=crc.LONG_K, epsAbs=0.0, epsRel=0.0)
    perm = c_oracle.kkt_ordering(P, A)
    spread = dict(rho=0.0, x=0.0, z=0.0, y=0.0)
    for b in range(3):
        xc, io = c_oracle.solve(P, Q[b], A, L[b], U[b], linsys=c_oracle.KIND_CG_MATFREE, epsPcg=1e-13, numItrPcg=5000, **kw)
        xl, il = c_oracle.solve(P, Q[b], A, L[b], U[b], linsys=c_oracle.KIND_KKT_LDL_SPARSE, perm=perm, **kw)
        margin = crc.switch_margin(io["rhoFinal"] / crc.LONG_RHO, 5.0)
        print(f"column {b}: numRefactor {io['numRefactor']}/{il['numRefactor']} rhoFinal {io['rhoFinal']:.6g} margin {margin:.3f}")
        assert io["numRefactor"] == il["numRefactor"] == 1 and io["iterations"] == crc.LONG_K and margin >= crc.LONG_CLEAR
        for q, v in (("rho", abs(io["rhoFinal"] - il["rhoFinal"]) / il["rhoFinal"]), ("x", rel(xc, xl)), ("z", rel(io["z"], il["z"])), ("y", rel(io["y"], il["y"]))):
            spread[q] = max(spread[q], v)
    print("long: spread CG against L D L': " + " ".join(f"{q} {v:.1e}" for q, v in spread.items()) + f"; table {crc.LONG_SPREAD}")
    assert all(spread[q] <= max(2.0 * crc.LONG_SPREAD[q], 1e-12) for q in spread), spread


@pytest.mark.parametrize("kind", list(crc.COMPOSE))
def test_composition_rows_are_clear(kind):
    """The rows of the composition tests (equality scale; warm-started re-solve): both forms of the restatement take the same switches on the compared columns,
    some column switches, column 2 -- the one with equality rows -- is compared, and the two forms agree to the recorded spread."""
    kkt, red = crc.compose_run(kind), crc.compose_run(kind, "reduced")
    keep = crc.compared(kkt)
    print(f"{kind}: compared {keep}; switches {[[s[0] for s in kkt[b]['switches']] for b in keep]}")
    assert len(keep) >= crc.COUNT - crc.MAX_LEFT_OUT and 2 in keep
    spread = dict(rho=0.0, x=0.0, z=0.0, y=0.0)
    for b in keep:
        assert [s[0] for s in kkt[b]["switches"]] == [s[0] for s in red[b]["switches"]], b
        for q, v in (("rho", abs(kkt[b]["rhoFinal"] - red[b]["rhoFinal"]) / red[b]["rhoFinal"]), ("x", rel(kkt[b]["x"], red[b]["x"])),
                     ("z", rel(kkt[b]["z"], red[b]["z"])), ("y", rel(kkt[b]["y"], red[b]["y"]))):
            spread[q] = max(spread[q], v)
    print(f"{kind}: spread reduced against kkt: " + " ".join(f"{q} {v:.1e}" for q, v in spread.items()) + f"; table {crc.COMPOSE[kind]}")
    assert all(spread[q] <= max(2.0 * crc.COMPOSE[kind][q], 1e-12) for q in spread), spread
    assert sum(kkt[b]["numRefactor"] > 0 for b in keep) >= 2
