"""Cases and references of the polishing step on the shared-matrix batches (qps_polish_shared, qps_set_shared_polish): what tests/test_shared_polish_cpu.py guards
and tests/test_gpu_shared_polish.py runs on the device.

The reference is oracle/polish_oracle_np.py::Polish per column and a direct solve of K t = g on the active rows.  Parity tests hand the SAME (X, Y) to both sides, Y
thresholded at |y| > 1e-7 (tests/test_gpu_polish.py); MINRES iteration counts are never compared with the restatement.  Everything here is computed once per process
and shared; nobody changes what these functions return."""
import functools

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from equilibration_cases import ruiz_pow2, scrambled_family
from oracle import polish_oracle_np, qps_oracle_np
from shared_batch_cases import shared_family
from sparse_shared_cases import lasso_path, random_family

Y_THRESHOLD = 1e-7
PARITY = dict(numItrPolish=10, δ=1e-6, ϵMinres=1e-9, numItrMinres=4000)       # the settings of the parity tests
PARITY_COLUMNS = {3: (0, 1, 2), 20: (0, 1, 2, 15, 16, 19), 37: (0, 15, 16, 31, 32, 36)}   # the columns compared with Polish, per count of shared_family(96, 160, .)
FLAG_CAP = 500                     # numItrMinres of the per-column flag test on shared_family(96, 160, 20): columns 0 and 2 need more on their first call
FLAG_COLUMNS_OVER = (0, 2)
EQUIL_PASSES = 10

# The staged kernel form: shared_family(2112, 2304, 37) puts P (2112 x 2112 is below, A and A' at 2112 x 2304 doubles = 37.1 MiB are above) past the 32 MiB cut of
# the cached form and gives two panels per workgroup.  Settings of the test, and on columns 2, 16 and 36 what the restatement does from the ORACLE's state:
# (MINRES iterations, max|x_r - t_direct|, max|x_admm - t_direct|), produced by
#     python -c "import sys; sys.path[:0] = ['.', 'tests']; import shared_polish_cases as c; print(c.staged_restatement())"
STAGED = dict(n=2112, m=2304, count=37, columns=(2, 16, 36), polish=dict(numItrPolish=1, δ=1e-6, ϵMinres=1e-6, numItrMinres=12000))
STAGED_RESTATEMENT = {2: (3262, 2.41e-7, 1.62e-5), 16: (2248, 2.16e-7, 5.09e-6), 36: (2164, 3.40e-7, 1.03e-5)}     # flag 0 on all three


MAX_COUNT = {"dense": 37, "random": 37, "scrambled": 4, "staged": 37}   # column b of a family is the same for every count: states are taken from the largest


def _dense(M):
    return np.asarray(M.toarray() if sp.issparse(M) else M, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def family(name, count):
    """(P, A, Q, L, U), P and A dense: "dense" = shared_family(96, 160, count), "random" = random_family(count), "scrambled" = scrambled_family(96, 160, count),
    "staged" = shared_family(2112, 2304, count).  Column b of a family does not depend on count."""
    P, A, Q, L, U = {"dense": lambda: shared_family(96, 160, count), "random": lambda: random_family(count), "scrambled": lambda: scrambled_family(96, 160, count),
                     "staged": lambda: shared_family(STAGED["n"], STAGED["m"], count)}[name]()
    return _dense(P), _dense(A), Q, L, U


def threshold(Y):
    return np.where(np.abs(Y) > Y_THRESHOLD, Y, 0.0)


@functools.lru_cache(maxsize=None)
def state(name, b):
    """(x, y raw) of column b after the restatement's ADMM loop to 1e-4 at a fixed rho = 0.1."""
    P, A, Q, L, U = family(name, MAX_COUNT[name])
    x = np.zeros(P.shape[0]); info = {}
    qps_oracle_np.SolveQuadraticProgramRefLoop(x, P, Q[b], A, L[b], U[b], qps_oracle_np.RedCholInit, qps_oracle_np.RedChol, numIterations=4000, εAbs=1e-4, εRel=1e-4,
                                               ρ=0.1, adptΡ=False, info=info)
    return x, np.asarray(info["y"], dtype=np.float64)


def states(name, count):
    """(X [count x n], Y [count x m] thresholded) of a whole family."""
    S = [state(name, b) for b in range(count)]
    return np.ascontiguousarray(np.stack([s[0] for s in S])), np.ascontiguousarray(threshold(np.stack([s[1] for s in S])))


def direct(P, q, A, l, u, y):
    """x of the solution of K t = g on the active rows of y (sparse P and A: a sparse LU)."""
    Lo, Up = y < 0, y > 0
    n = P.shape[0]
    if sp.issparse(P):
        A = sp.csr_matrix(A)
        Aa = sp.vstack([A[np.flatnonzero(Lo)], A[np.flatnonzero(Up)]])
        K = sp.bmat([[sp.csc_matrix(P), Aa.T], [Aa, None]], format="csc")
        return spla.splu(K).solve(np.concatenate([-q, l[Lo], u[Up]]))[:n]
    Aa = np.vstack([A[Lo], A[Up]])
    return np.linalg.solve(np.block([[P, Aa.T], [Aa, np.zeros((Aa.shape[0],) * 2)]]), np.concatenate([-q, l[Lo], u[Up]]))[:n]


@functools.lru_cache(maxsize=None)
def direct_of(name, b):
    P, A, Q, L, U = family(name, MAX_COUNT[name])
    return direct(P, Q[b], A, L[b], U[b], threshold(state(name, b)[1]))


@functools.lru_cache(maxsize=None)
def restatement(name, b, numItrPolish=10, δ=1e-6, ϵMinres=1e-9, numItrMinres=4000):
    """Polish on the thresholded oracle state of column b: (x_r, flag, info)."""
    P, A, Q, L, U = family(name, MAX_COUNT[name])
    x, y = state(name, b)
    return polish_oracle_np.Polish(P, Q[b], A, L[b], U[b], x, threshold(y), numItrPolish, δ, ϵMinres, numItrMinres)


def _polish(P, q, A, l, u, x, y, *, numItrPolish, δ, ϵMinres, numItrMinres):
    return polish_oracle_np.Polish(P, q, A, l, u, x, y, numItrPolish, δ, ϵMinres, numItrMinres)


def first_call_iterations(name, b):
    """MINRES iterations of the restatement's first call at the parity tolerance (numItrPolish = 1)."""
    return restatement(name, b, 1, 1e-6, 1e-9, 4000)[2]["minresIterations"]


@functools.lru_cache(maxsize=None)
def equilibrated(count=4):
    """scrambled_family(96, 160, count) and D, E of ten passes of the power-of-two rule (what get_equilibration() of the handle returns)."""
    P, A, Q, L, U = family("scrambled", count)
    kd, ke = ruiz_pow2(P, A, EQUIL_PASSES)
    return (P, A, Q, L, U), np.ldexp(1.0, np.asarray(kd, dtype=np.int64)), np.ldexp(1.0, np.asarray(ke, dtype=np.int64))


def equilibrated_restatement(b, D, E, X, Y, numItrMinres=4000):
    """Polish on the scaled data from the scaled state, times D: what the handle computes with the equilibration on."""
    (P, A, Q, L, U), _, _ = equilibrated()
    xr, flag, info = polish_oracle_np.Polish(P * np.outer(D, D), D * Q[b], A * np.outer(E, D), E * L[b], E * U[b], X[b] / D, Y[b] / E, 10, 1e-6, 1e-9, numItrMinres)
    return D * xr, flag, info


def staged_restatement():
    """The figures of STAGED_RESTATEMENT, per column (flag, MINRES iterations, max|x_r - t_direct|, max|x_admm - t_direct|); a few minutes on a CPU."""
    out = {}
    for b in STAGED["columns"]:
        P, A, Q, L, U = family("staged", MAX_COUNT["staged"])
        x, y = state("staged", b)
        xr, flag, info = _polish(P, Q[b], A, L[b], U[b], x, threshold(y), **STAGED["polish"])
        t = direct_of("staged", b)
        out[b] = (flag, info["minresIterations"], float(np.abs(xr - t).max()), float(np.abs(x - t).max()))
    return out
