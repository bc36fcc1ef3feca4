"""CPU-only checks of the opt-in warm start of z and y of the shared-matrix batches (qps_set_shared_warm_start, qps_set_shared_dual): both symbols are declared,
exported and bound in header, library, ctypes and Julia; a NULL handle and a bad mode are refused without a device; the numpy restatement of
tests/warm_start_cases.py -- the reference of the GPU tests -- splits exactly (50 iterations, then 50 more from the returned state, are 100 iterations); and
every row of the case table is reproduced by both linear-system forms with no stopping decision on a rounding edge."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from equilibration_cases import EquilibratedRestatement, scrambled_family, warm_start
from family_rho_cases import FamilyRestatement
from warm_start_cases import CASES, STEPS, WarmRestatement, dense, family, sequence_data, sequence_run, step

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARGUMENT = 1


def test_symbols_are_declared_exported_and_bound(qps):
    from quadraticprogramsolver_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qps.h")).read(), flags=re.S)
    assert re.search(r"\bint32_t\s+qps_set_shared_warm_start\s*\(\s*qps_handle\s+\w+\s*,\s*int32_t\s+\w+\s*\)\s*;", header)
    assert re.search(r"\bint32_t\s+qps_set_shared_dual\s*\(\s*qps_handle\s+\w+\s*,\s*const\s+double\s*\*\s*\w+\s*,\s*const\s+double\s*\*\s*\w+\s*\)\s*;", header)
    jl = re.sub(r"#[^\n]*", "", open(os.path.join(ROOT, "julia", "QuadraticProgramSolverHIP.jl"), encoding="utf-8").read())
    assert re.search(r"ccall\(\(:qps_set_shared_warm_start,\s*LIBQPS\),\s*Int32,\s*\(Ptr\{Cvoid\},\s*Int32\)", jl)
    assert re.search(r"ccall\(\(:qps_set_shared_dual,\s*LIBQPS\),\s*Int32,\s*\(Ptr\{Cvoid\},\s*Ptr\{Float64\},\s*Ptr\{Float64\}\)", jl)
    dp = C.POINTER(C.c_double)
    for name, args in (("qps_set_shared_warm_start", [C.c_void_p, C.c_int32]), ("qps_set_shared_dual", [C.c_void_p, dp, dp])):
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(C.CDLL(_lib.LIB_PATH), name), f"{name} is not exported by the library"
        fn = getattr(_lib.lib(), name)
        assert fn.restype is C.c_int32 and list(fn.argtypes) == args
    for method in ("set_warm_start", "set_dual"):
        assert getattr(qps.QuadraticProgramSparseSharedBatch, method) is getattr(qps.QuadraticProgramSharedBatch, method)


def test_null_handle_and_bad_mode_are_refused_without_a_device(qps):
    from quadraticprogramsolver_amd import _lib
    L = _lib.lib()
    for mode in (0, 1, 2, 3, -1):
        assert L.qps_set_shared_warm_start(None, mode) == BAD_ARGUMENT
    assert b"NULL" in L.qps_last_error(None)
    z = np.zeros(4)
    ptr = z.ctypes.data_as(C.POINTER(C.c_double))
    assert L.qps_set_shared_dual(None, ptr, ptr) == BAD_ARGUMENT and L.qps_set_shared_dual(None, None, None) == BAD_ARGUMENT


def test_python_mode_names(qps):
    """None / False / "off" -> 0, True / "state" -> 1, "ax" -> 2; anything else is refused before the library is asked."""
    modes = qps.QuadraticProgramSharedBatch._WARM_MODES
    assert [modes[k] for k in (None, False, "off", True, "state", "ax")] == [0, 0, 0, 1, 1, 2]

    class Probe(qps.QuadraticProgramSharedBatch):          # no handle: only the argument handling runs
        def __init__(self):
            self._h = None

        def close(self):
            pass

    with pytest.raises(ValueError):
        Probe().set_warm_start("warm")


@pytest.mark.parametrize("form", ["reduced", "kkt"])
def test_the_restatement_splits_exactly(form):
    """eps = 0: 50 iterations cold, then 50 from the returned (x, z, y), are the 100 iterations of one cold run -- xp and zp restart at 0 and are overwritten by
    iteration 1 before anything reads them, so nothing but (x, z, y) carries over."""
    P, A, Q, L, U = family("shared", 96, 160, 4)
    R = WarmRestatement(P, A, form=form)
    kw = dict(epsAbs=0.0, epsRel=0.0)
    whole = R.solve_from(Q, L, U, numIterations=100, **kw)
    half = R.solve_from(Q, L, U, numIterations=50, **kw)
    rest = R.solve_from(Q, L, U, half["X"], half["Z"], half["Y"], numIterations=50, **kw)
    for k in ("X", "Z", "Y"):
        assert np.array_equal(rest[k], whole[k]), k
    assert not np.array_equal(half["X"], whole["X"])
    assert [c["iterations"] for c in rest["columns"]] == [50] * 4 and [c["convFlag"] for c in rest["columns"]] == [1] * 4


def test_from_zero_state_it_is_the_family_restatement():
    """solve_from with no state is FamilyRestatement.solve with the fixed rho, bit for bit (passes = 0 makes D = E = 1), and with a scaling it is
    EquilibratedRestatement.solve, warm start of x included."""
    P, A, Q, L, U = family("shared", 96, 160, 4)
    a = WarmRestatement(P, A, form="reduced").solve_from(Q, L, U, numIterations=60, epsAbs=0.0, epsRel=0.0)
    b = FamilyRestatement(P, A, form="reduced").solve(Q, L, U, numIterations=60, epsAbs=0.0, epsRel=0.0, adaptive=False)
    Ps, As, Qs, Ls, Us = scrambled_family(96, 160, 4)
    X0 = warm_start(Qs)
    c = WarmRestatement(Ps, As, 10, form="reduced").solve_from(Qs, Ls, Us, X0, numIterations=60, epsAbs=0.0, epsRel=0.0)
    d = EquilibratedRestatement(Ps, As, 10, form="reduced").solve(Qs, Ls, Us, X0=X0, numIterations=60, epsAbs=0.0, epsRel=0.0)
    for p, q in ((a, b), (c, d)):
        for i in range(4):
            assert all(np.array_equal(p["columns"][i][k], q["columns"][i][k]) for k in ("x", "z", "y"))
            assert (p["columns"][i]["resPrim"], p["columns"][i]["resDual"]) == (q["columns"][i]["resPrim"], q["columns"][i]["resDual"])


def test_step_is_deterministic_and_keeps_the_bound_pattern():
    P, A, Q, L, U = family("random", 20)
    a, b = step(Q, L, U, 2), step(Q, L, U, 2)
    assert all(np.array_equal(p, q) for p, q in zip(a, b))
    assert not np.array_equal(a[0], step(Q, L, U, 3)[0]) and not np.array_equal(a[0], Q)
    assert np.array_equal(np.isinf(a[1]), np.isinf(L)) and np.array_equal(np.isinf(a[2]), np.isinf(U))
    assert np.array_equal(a[1] == a[2], L == U)            # l and u move together: equalities stay equalities
    assert np.abs(a[0] - Q).max() <= 0.02 * np.mean(np.abs(Q)) * 6 and len(sequence_data("random20")) == STEPS + 1


@pytest.mark.parametrize("name", list(CASES))
def test_case_table_and_rounding_guard(name):
    """Both forms reproduce the row -- flags and stopping iterations of the cold solve and of every warm re-solve -- and a GPU test cannot hide a decision that sits
    on a rounding edge: at every column's stopping check and at the check before it, each deciding quotient (residual / threshold, and the two difference norms /
    epsAdmm of the stall test) is further than 1e-3 from 1.  The device is held to 1e-9 on the iterates, six orders below."""
    c = CASES[name]
    edges = []
    for form in ("reduced", "kkt"):
        runs = sequence_run(name, form)
        assert [[k["iterations"] for k in r["columns"]] for r in runs] == c["iterations"], form
        assert [[k["convFlag"] for k in r["columns"]] for r in runs] == c["flags"], form
        edge = min(abs(q - 1.0) for r in runs for t in r["trace"] for _, qs in t[-2:] for q in qs)
        print(f"{name} {form}: closest deciding quotient to 1 at a stopping check or the check before: {edge:.2e}")
        assert edge > 1e-3
        edges.append(edge)
        cold = sequence_run(name, form, warm=False)
        assert [[k["iterations"] for k in r["columns"]] for r in cold] == c["x_only"], form
    assert abs(edges[0] - edges[1]) <= 1e-6                # the two forms agree in the figure itself
    warm_total, cold_total = (sum(sum(r) for r in c[k][1:]) for k in ("iterations", "x_only"))
    print(f"{name}: sum of iterations over the re-solves, from (x, z, y) {warm_total}, from x alone {cold_total}")


def test_mode_two_is_a_state_with_z_equal_to_a_x():
    """What the handles do in mode 2, said in the helper's terms: Z0 = X0 A' with the caller's A, whatever the scaling."""
    Ps, As, Qs, Ls, Us = scrambled_family(96, 160, 4)
    X0 = warm_start(Qs)
    Y0 = 0.05 * np.random.default_rng(3).standard_normal(Ls.shape)
    R = WarmRestatement(Ps, As, 10, form="reduced")
    r = R.solve_from(Qs, Ls, Us, X0, X0 @ dense(As).T, Y0, numIterations=1, epsAbs=0.0, epsRel=0.0)
    # one iteration by hand in the scaled variables
    D, E = R.D[:, None], R.E[:, None]
    X, Z, Y = X0.T / D, (dense(As) @ X0.T) * E, Y0.T / E
    R._factorize(0.1)
    XX, ZZ = R._linsys(X, Qs.T * D, Z, Y)
    Zn = np.clip(1.6 * ZZ - 0.6 * Z + Y / 0.1, Ls.T * E, Us.T * E)
    assert np.allclose(r["Z"], (Zn / E).T, rtol=1e-13, atol=0) and np.allclose(r["X"], ((1.6 * XX - 0.6 * X) * D).T, rtol=1e-13, atol=1e-300)
