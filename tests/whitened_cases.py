"""Cases of the whitened two-launch iteration (quadraticprogramsolver_amd/csrc/k_pass_w.hip) and its restatement in numpy, shared by
tests/test_gpu_whitened.py and tests/test_whitened_cpu.py.

A dense fp64 handle that solves on its cached factor (``reuseFactor=True``, fixed ρ) with QPS_WHITEN=1 carries u = W t, p = W x and a = A x
(W = inv(L), L L' = P + σ I + ρ A'A) and runs one stacked pass over [B ; tril(G)] (B = A W', G = W W') plus one slab sum per iteration.

The shapes lie above the single-launch kernel's domain and cover, with NP = roundup(n, 64) and 1024 columns per chunk of a 512-thread workgroup:
  (200, 330)    KC 1, NP = 256: 64 triangle tiles of 4 rows for 256 workgroups (most take none), ragged n and m
  (1100, 2130)  KC 2, NP = 1152, top chunk live (columns 1024 .. 1151), 12 rows of B per workgroup and a ragged last one
  (2100, 300)   KC 4, NP = 2112, top chunk live; MP = 320: 80 workgroups have rows of B, 176 write a zero slab of B'w
  (4100, 70)    KC 8, NP = 4160, top chunk live; MP = 128: 32 workgroups have rows of B
"""
import numpy as np
import scipy.linalg as sla

from quadraticprogramsolver_amd import GenerateDenseBenchmarkQP

SHAPES = [(200, 330), (1100, 2130), (2100, 300), (4100, 70)]
IDS = [f"n{n}_m{m}" for n, m in SHAPES]
STREAM = 21
K, PERIOD = 60, 10
BASE = dict(rho=1.0, sigma=1e-6, alpha=1.6)                              # the defaults of the reference signature (SolveQuadraticProgram.jl:15-17)
OFF_DEFAULT = [(1.9, 1e-2), (0.5, 1.0)]                                  # (α, σ)
OTHER_RHO = 0.3
TO_EPS = dict(numIterations=4000, numItrConv=25, epsAbs=1e-6, epsRel=1e-6, rho=0.1, sigma=1e-6, alpha=1.6)
# The stall stop (convAdmm, :105-107): every row an equality l = u = t with more rows than variables, so the residuals stay O(1), convPrimDual never fires, z = t
# from the first iteration on (|z - zp| = 0) and the run ends at the first check at which |x - xp| <= ϵAdmm = 1e-6 -- decided by the step norm alone, which the
# whitened loop evaluates as |L (p - pp)|
STALL = dict(numIterations=8000, numItrConv=25, epsAbs=1e-2, epsRel=1e-4, rho=0.1, sigma=1e-6, alpha=1.6)
FIELDS = ("x", "z", "y", "resPrim", "resDual")

_problems, _refs = {}, {}


def problem(shape, stall=False):
    """(mP, vQ, mA, vL, vU) of a shape: the feasible draw of the benchmark generator; stall: its rows turned into equalities nothing satisfies.
    Cached; treat as read-only."""
    if shape not in _problems:
        _problems[shape] = GenerateDenseBenchmarkQP(shape[0], shape[1], stream=STREAM, feasible=True)
    if stall:
        P, q, A, _, _ = _problems[shape]
        t = 0.5 * np.random.default_rng(56).standard_normal(shape[1])
        return P, q, A, t, t.copy()
    return _problems[shape]


def start(shape):
    """A non-zero x0."""
    return 0.3 * np.random.default_rng(55).standard_normal(shape[0])


def fixed_k(**over):
    return dict(dict(numIterations=K, numItrConv=PERIOD, epsAbs=0.0, epsRel=0.0, **BASE), **over)


def reference(co, shape, x0=None, stall=False, **params):
    """c_oracle.solve of a case, computed once per (shape, start, parameters) and shared: dict of x, z, y, resPrim, resDual, convFlag, iterations."""
    key = (shape, x0 is not None, stall, tuple(sorted(params.items())))
    if key not in _refs:
        P, q, A, l, u = problem(shape, stall)
        x, info = co.solve(P, q, A, l, u, vX=None if x0 is None else x0, **params)
        _refs[key] = dict(x=x, z=info["z"], y=info["y"], resPrim=info["resPrim"], resDual=info["resDual"], convFlag=info["convFlag"],
                          iterations=info["iterations"])
    return _refs[key]


def rel(a, b):
    a, b = np.atleast_1d(np.asarray(a, dtype=float)), np.atleast_1d(np.asarray(b, dtype=float))
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))


def whitened_loop(P, q, A, l, u, x0=None, *, numIterations, numItrConv, epsAbs, epsRel, rho, sigma, alpha):
    """The recurrences of the whitened loop as the kernels run them: the stacked pass (z~ = B u, row updates, a+ = α z~ + (1 - α) a, B'w; the triangle
    of G as row dots d plus the column sums of its strictly lower part), the slab sum (p+, u+), and at a check the three products with L."""
    n, m = P.shape[0], A.shape[0]
    L = np.linalg.cholesky(P + sigma * np.eye(n) + rho * (A.T @ A))
    W = sla.solve_triangular(L, np.eye(n), lower=True)
    B, G, c = A @ W.T, W @ W.T, W @ q
    Gd, Gs = np.tril(G), np.tril(G, -1)
    x = np.zeros(n) if x0 is None else np.array(x0, dtype=float)
    p, a = W @ x, A @ x
    z, y = np.zeros(m), np.zeros(m)
    alpha1, rho1 = 1 - alpha, 1 / rho
    eps_admm = min(epsAbs, epsRel) * 1e-2
    flag, res, ii, steps = 1, (np.nan, np.nan), 0, []
    uu = sigma * p - c                                                   # z = y = 0: no slabs for the first right-hand side
    for ii in range(1, numIterations + 1):
        zt = B @ uu
        g = Gd @ uu + Gs.T @ uu
        zo = z
        z = np.clip(alpha * zt + alpha1 * zo + rho1 * y, l, u)
        y = y + rho * (alpha * zt + alpha1 * zo - z)
        a = alpha * zt + alpha1 * a
        e = B.T @ (rho * z - y)
        pp = p
        p = alpha * g + alpha1 * pp
        uu = sigma * p - c + e
        if ii % numItrConv == 0:
            x, dx, Aty = L @ p, L @ (p - pp), L @ (B.T @ y)
            Px = P @ x
            inf = lambda v: float(np.abs(v).max()) if v.size else 0.0
            steps.append(inf(dx))
            res = (inf(a - z), inf(Px + q + Aty))
            if res[0] < epsAbs + epsRel * max(inf(a), inf(z)) and res[1] < epsAbs + epsRel * max(inf(Px), inf(Aty), inf(q)):
                flag = 3
            if inf(dx) <= eps_admm and inf(z - zo) <= eps_admm:
                flag = 2
            if flag != 1:
                break
    return dict(x=L @ p, z=z, y=y, resPrim=res[0], resDual=res[1], convFlag=flag, iterations=ii, a=a, A_x=A @ (L @ p), steps=steps)
