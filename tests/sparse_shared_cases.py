"""Families of QPs that share a SPARSE mP and mA and differ in q, l, u only: what tests/test_sparse_shared_cpu.py, tests/test_gpu_sparse_shared_batch.py and
tests/tools/gpu_sparse_shared_batch_timing.py solve on a sparse shared-matrix batch handle (qps_create_csc_shared_batch)."""
import numpy as np

from quadraticprogramsolver_amd.generator import GenerateRandomQP, ProblemClass, make_rng


def lasso_path(numElements, count):
    """A regularisation path: the lasso problem of GenerateRandomQP(lassoOptimization, numElements, rng=make_rng(77, 6)) with the weight lambda -- the
    last numElements entries of q -- set to lambda_max (0.05 + 0.95 b / (count - 1)) in column b, lambda_max = 5 q[-1]; l and u repeated.
    Returns (mP, mA, mQ [count x N], mL [count x M], mU [count x M])."""
    P, q, A, l, u = GenerateRandomQP(ProblemClass.lassoOptimization, numElements, rng=make_rng(77, 6))
    lam_max = 5.0 * q[-1]
    Q = np.tile(q, (count, 1))
    for b in range(count):
        Q[b, -numElements:] = lam_max * (0.05 + 0.95 * b / max(count - 1, 1))
    return P, A, Q, np.tile(l, (count, 1)), np.tile(u, (count, 1))


def random_family(count):
    """mP and mA of GenerateRandomQP(randomQp, 100, rng=make_rng(77, 1)) (n = 100, m = 50); per column b, from make_rng(78, 1): q ~ N(0,1),
    x0 ~ N(0,1)/sqrt(n), s = A x0, l = s - (1 + b) U(0,1), u = s + (1 + b) U(0,1) (x0 is feasible).  Column 1 has l = -Inf."""
    P, _, A, _, _ = GenerateRandomQP(ProblemClass.randomQp, 100, rng=make_rng(77, 1))
    n, m = P.shape[0], A.shape[0]
    rng = make_rng(78, 1)
    Q, L, U = np.zeros((count, n)), np.zeros((count, m)), np.zeros((count, m))
    for b in range(count):
        Q[b] = rng.standard_normal(n)
        x0 = rng.standard_normal(n) / np.sqrt(n)
        s = A @ x0
        L[b] = s - (1 + b) * rng.random(m)
        U[b] = s + (1 + b) * rng.random(m)
        if b == 1:
            L[b] = -np.inf
    return P, A, Q, L, U


# the stopping iterations of the C oracle (linsys = KIND_KKT_LDL_SPARSE, rho = 0.1, eps = 1e-6, 5000 iterations) on random_family(20); every column ends with flag 3
RANDOM_FAMILY_ORACLE_ITERATIONS = [200, 75, 75, 100, 50, 50, 100, 50, 75, 50, 75, 50, 50, 75, 75, 50, 75, 50, 50, 50]
