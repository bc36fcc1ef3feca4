"""CPU-only checks of the per-constraint rho scale (qps_set_shared_rho_scale): the symbol is declared, exported and bound in all three places, a NULL
handle is refused without a device, the scale builders give what they say, and the numpy restatement of tests/rho_scale_cases.py -- the reference of the
GPU tests -- agrees with itself in its two forms and, at s = 1, with the C oracle's fixed-rho solve."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from rho_scale_cases import Restatement, pattern_rho_scale, scale_of
from shared_batch_cases import shared_family
from sparse_shared_cases import lasso_path, random_family

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "qps_set_shared_rho_scale"
BAD_ARGUMENT = 1


def rel(a, b):
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


def test_symbol_is_declared_exported_and_bound(qps):
    from quadraticprogramsolver_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qps.h")).read(), flags=re.S)
    assert re.search(r"\bint32_t\s+%s\s*\(\s*qps_handle\s+\w+\s*,\s*const\s+double\s*\*\s*\w+\s*\)" % NAME, header), f"{NAME} is not declared in include/qps.h"
    assert NAME in _lib.EXPORTED_SYMBOLS
    assert hasattr(C.CDLL(_lib.LIB_PATH), NAME), f"{NAME} is not exported by the library"
    fn = getattr(_lib.lib(), NAME)
    assert fn.restype is C.c_int32 and list(fn.argtypes) == [C.c_void_p, C.POINTER(C.c_double)]
    jl = re.sub(r"#[^\n]*", "", open(os.path.join(ROOT, "julia", "QuadraticProgramSolverHIP.jl"), encoding="utf-8").read())
    assert re.search(r"ccall\(\(:%s,\s*LIBQPS\),\s*Int32,\s*\(Ptr\{Cvoid\},\s*Ptr\{Float64\}\)" % NAME, jl), f"{NAME} has no ccall in the Julia binding"
    assert hasattr(qps.QuadraticProgramSharedBatch, "set_rho_scale")
    assert qps.QuadraticProgramSparseSharedBatch.set_rho_scale is qps.QuadraticProgramSharedBatch.set_rho_scale
    assert "equality_rho_scale" in qps.__all__


def test_null_handle_is_refused_without_a_device(qps):
    from quadraticprogramsolver_amd import _lib
    L = _lib.lib()
    s = np.ones(4)
    assert L.qps_set_shared_rho_scale(None, s.ctypes.data_as(C.POINTER(C.c_double))) == BAD_ARGUMENT
    assert b"NULL" in L.qps_last_error(None)
    assert L.qps_set_shared_rho_scale(None, None) == BAD_ARGUMENT


def test_scale_builders(qps):
    L = np.array([[0.0, 1.0, -np.inf, 2.0, 5.0], [0.0, 1.5, -np.inf, 2.0, 5.0]])
    U = np.array([[0.0, 1.0, np.inf, 3.0, 5.0], [0.0, 1.5, np.inf, 2.0, 6.0]])
    # row 0 and row 1: l == u in every column (row 1 with a different value per column); row 3 and row 4 are equalities in ONE column only
    assert np.array_equal(qps.equality_rho_scale(L, U), [1e3, 1e3, 1.0, 1.0, 1.0])
    assert np.array_equal(qps.equality_rho_scale(L[1], U[1], factor=50), [50.0, 50.0, 1.0, 50.0, 1.0])
    with pytest.raises(ValueError):
        qps.equality_rho_scale(L, U[:, :-1])
    s = pattern_rho_scale(9)
    assert np.array_equal(s, [1000.0, 8.0, 1.0, 0.25, 1000.0, 8.0, 1.0, 0.25, 1000.0])
    assert set(pattern_rho_scale(160)) == {0.25, 1.0, 8.0, 1000.0}
    # the equality scale of the test families is not trivial: shared_family has equality rows and inequality rows, lasso is mostly equalities
    _, _, _, L, U = shared_family(96, 160, 3)
    eq = qps.equality_rho_scale(L, U)
    assert 0 < (eq == 1e3).sum() < 160
    _, _, _, L, U = lasso_path(10, 3)
    eq = qps.equality_rho_scale(L, U)
    assert (eq == 1e3).sum() == 1000 and eq.size == 1020


@functools.lru_cache(maxsize=None)
def _family(name):
    return {"shared96": lambda: shared_family(96, 160, 2), "shared200": lambda: shared_family(200, 330, 2), "lasso10": lambda: lasso_path(10, 2),
            "lasso20": lambda: lasso_path(20, 2), "random": lambda: random_family(2)}[name]()


@pytest.mark.parametrize("kind", ["equality", "pattern"])
@pytest.mark.parametrize("name,K", [("shared96", 100), ("shared200", 100), ("lasso10", 60), ("lasso20", 60), ("random", 60)])
def test_the_two_forms_of_the_restatement_agree(qps, name, K, kind):
    """Reduced Cholesky against dense KKT LU, the iterates after K iterations: measured <= 6e-12 relative on x, z, y over these cases (lasso20, pattern scale); 1e-10 asserted."""
    P, A, Q, L, U = _family(name)
    s = scale_of(kind, L, U)
    red, kkt = Restatement(P, A, s, form="reduced"), Restatement(P, A, s, form="kkt")
    for b in range(2):            # random_family / shared_family: column 1 has l = -Inf
        kw = dict(numIterations=K, epsAbs=0.0, epsRel=0.0)
        a, c = red.solve(Q[b], L[b], U[b], **kw), kkt.solve(Q[b], L[b], U[b], **kw)
        fig = [rel(a[k], c[k]) for k in "xzy"]
        print(f"{name} {kind} column {b}: reduced vs kkt rel x {fig[0]:.2e} z {fig[1]:.2e} y {fig[2]:.2e}")
        assert max(fig) <= 1e-10
        assert a["iterations"] == c["iterations"] == K and a["convFlag"] == c["convFlag"] == 1


def test_unit_scale_is_the_oracles_fixed_rho_solve(c_oracle):
    """s = 1 is the scalar loop: both forms against the C oracle at rho = 0.1, iterates at a fixed K within the bounds two fp64 implementations of this loop are
    held to elsewhere in the suite (1e-9 on x and z, 1e-8 on y), and flag and stopping iteration to eps = 1e-6."""
    P, A, Q, L, U = _family("shared96")
    red = Restatement(P, A, np.ones(A.shape[0]), form="reduced")
    for b in range(2):
        xo, io = c_oracle.solve(P, Q[b], A, L[b], U[b], rho=0.1, numIterations=100, epsAbs=0.0, epsRel=0.0)
        r = red.solve(Q[b], L[b], U[b], numIterations=100, epsAbs=0.0, epsRel=0.0)
        assert rel(r["x"], xo) <= 1e-9 and rel(r["z"], io["z"]) <= 1e-9 and rel(r["y"], io["y"]) <= 1e-8
        assert abs(r["resPrim"] - io["resPrim"]) <= 1e-9 * max(1.0, io["resPrim"]) and abs(r["resDual"] - io["resDual"]) <= 1e-9 * max(1.0, io["resDual"])
        xo, io = c_oracle.solve(P, Q[b], A, L[b], U[b], rho=0.1, numIterations=5000, epsAbs=1e-6, epsRel=1e-6)
        r = red.solve(Q[b], L[b], U[b], numIterations=5000, epsAbs=1e-6, epsRel=1e-6)
        assert (r["convFlag"], r["iterations"]) == (io["convFlag"], io["iterations"])
        assert np.abs(r["x"] - xo).max() <= 1e-5
    P, A, Q, L, U = _family("random")
    kkt = Restatement(P, A, np.ones(A.shape[0]), form="kkt")
    for b in range(2):
        xo, io = c_oracle.solve(P, Q[b], A, L[b], U[b], rho=0.1, numIterations=60, epsAbs=0.0, epsRel=0.0, linsys=c_oracle.KIND_KKT_LDL_SPARSE)
        r = kkt.solve(Q[b], L[b], U[b], numIterations=60, epsAbs=0.0, epsRel=0.0)
        assert rel(r["x"], xo) <= 1e-9 and rel(r["z"], io["z"]) <= 1e-9 and rel(r["y"], io["y"]) <= 1e-8
