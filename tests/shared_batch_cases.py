"""Families of QPs that share mP and mA and differ in q, l, u only: what tests/test_gpu_shared_batch.py and
tests/tools/gpu_shared_batch_timing.py solve on a shared-matrix batch handle."""
import numpy as np

from quadraticprogramsolver_amd.generator import GenerateDenseBenchmarkQP, make_rng


def shared_family(n, m, count, *, seed=77, stream=3, inf_column=1):
    """mP, mA and the equality rows of GenerateDenseBenchmarkQP(n, m, stream=10, feasible=True); per column b: q ~ N(0,1), x0 ~ N(0,1)/sqrt(n),
    s = A x0, l / u = s -/+ (1 + b) U(0,1) on the inequality rows and s on the equality rows (x0 is feasible).  Column ``inf_column`` has
    l = -Inf on its inequality rows.  Returns (mP, mA, mQ [count x n], mL [count x m], mU [count x m])."""
    P, _, A, l0, u0 = GenerateDenseBenchmarkQP(n, m, stream=10, feasible=True)
    eq = l0 == u0
    rng = make_rng(seed, stream)
    Q, L, U = np.zeros((count, n)), np.zeros((count, m)), np.zeros((count, m))
    for b in range(count):
        Q[b] = rng.standard_normal(n)
        x0 = rng.standard_normal(n) / np.sqrt(n)
        s = A @ x0
        L[b] = np.where(eq, s, s - (1 + b) * rng.random(m))
        U[b] = np.where(eq, s, s + (1 + b) * rng.random(m))
        if b == inf_column:
            L[b] = np.where(eq, s, -np.inf)
    return P, A, Q, L, U
