#!/usr/bin/env python
"""What the opt-in infeasibility certificates (qps_set_shared_infeasibility) cost per check and buy per batch, on the shared-matrix batch handles.

Shapes:  dense  shared_family(2112, 2304, 37), fp64 (the staged kernel form, three panels), column 5 shifted by c = 12 against a null vector of A'
         sparse lasso_path(100, 16), fp64, the weight of column 7 negative, the family-wide rho rule on (fctrRho = 4)
Parts:
  cost   loop wall time (tLoop, one warm-up solve and three timed ones) with the option off and on, and -- every check bracketed by qps_set_profiling 2 -- the
         device time per check of the existing check category and of the new one.  Dense: the shifted family at rho = 1, K = 1000 (the column is not flagged there:
         the price of the option alone) and the unshifted family, K = 300; sparse: numIterations = 1000.
  sweep  dense only: fixed rho and the family rule at base rho 0.1 / 1 / 10, numIterations = 2000, option off and on: the flag and stopping iteration of the shifted
         column, the batch's longest run, how many columns took which flag, tLoop.
--tree DIR imports the package from another checkout (built there); one without the option (the parent commit) runs the option-off rows only.
Nothing is asserted: the figures are a record.

    python tests/tools/gpu_infeasibility_timing.py [--parts cost,sweep] [--tree DIR]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
EPS = dict(ϵAbs=1e-6, ϵRel=1e-6, numItrConv=25)


def null_vector(M, seed):
    """tests/infeasibility_cases.py: _null_vector (restated: a parent checkout does not have that file)."""
    import numpy as np
    r = np.random.default_rng(seed).standard_normal(M.shape[1])
    v = r - M.T @ np.linalg.lstsq(M.T, r, rcond=None)[0]
    v = v - M.T @ np.linalg.lstsq(M.T, v, rcond=None)[0]
    return v / np.linalg.norm(v)


def per_check(prob):
    out = {}
    for k in prob.kernel_times():
        for word in ("check (", "infeasibility ("):
            if word in k["name"]:
                out[word.rstrip(" (")] = f"{k['seconds'] / k['launches'] * 1e6:.1f} us x {k['launches']}"
    return out


def cost(label, make, have, kw):
    for on in ([False, True] if have else [False]):
        with make() as prob:
            if on:
                prob.set_infeasibility()
            prob.solve(**kw)
            loops = []
            for _ in range(3):
                _, flags, infos = prob.solve(**kw)
                loops.append(infos[0]["tLoop"] * 1e3)
            fl = [int(f) for f in flags]
            prob.set_profiling(2)
            prob.solve(**kw)
            figures = per_check(prob)
        print(f"{label}, option {'on ' if on else 'off'}: tLoop {min(loops):.2f} / {sorted(loops)[1]:.2f} / {max(loops):.2f} ms, longest run "
              f"{max(i['iterations'] for i in infos)}, flags {({k: fl.count(k) for k in sorted(set(fl))})}, per check {figures}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="cost,sweep")
    ap.add_argument("--tree", default=ROOT)
    args = ap.parse_args()
    tree = os.path.abspath(args.tree)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, tree)
    import numpy as np
    import quadraticprogramsolver_amd as qps
    from shared_batch_cases import shared_family
    from sparse_shared_cases import lasso_path
    assert os.path.abspath(qps.__file__).startswith(tree), qps.__file__
    have = hasattr(qps.QuadraticProgramSharedBatch, "set_infeasibility")
    print(f"tree {os.path.relpath(tree, ROOT)}: {'has' if have else 'does not have'} the option", flush=True)
    parts = args.parts.split(",")

    P, A, Q, L0, U0 = shared_family(2112, 2304, 37)
    v, b, c = null_vector(A.T, 5), 5, 12.0
    L, U = L0.copy(), U0.copy()
    L[b] -= c * np.sign(v)
    U[b] -= c * np.sign(v)
    print(f"dense: column {b} shifted by {c}: sum_(v>0) u v + sum_(v<0) l v = {np.sum(U[b][v > 0] * v[v > 0]) + np.sum(L[b][v < 0] * v[v < 0]):.1f}, "
          f"||A'v|| = {np.abs(A.T @ v).max():.1e}", flush=True)
    if "cost" in parts:
        cost("dense 2112 x 2304 x 37, column 5 infeasible, rho 1, K 1000", lambda: qps.QuadraticProgramSharedBatch(P, A, Q, L, U), have, dict(ρ=1.0, numIterations=1000, **EPS))
        cost("dense 2112 x 2304 x 37, all feasible, rho 1, K 300", lambda: qps.QuadraticProgramSharedBatch(P, A, Q, L0, U0), have, dict(ρ=1.0, numIterations=300, **EPS))
        Ps, As, Qs, Ls, Us = lasso_path(100, 16)
        Qs = Qs.copy()
        Qs[7, -100:] *= -1.0

        def make_lasso():
            prob = qps.QuadraticProgramSparseSharedBatch(Ps, As, Qs, Ls, Us)
            prob.set_adaptive_rho()
            return prob
        cost(f"lasso_path(100, 16) (N = {Ps.shape[0]}, M = {As.shape[0]}), column 7 unbounded, family rho from 0.1, numIterations 1000", make_lasso, have,
             dict(ρ=0.1, fctrΡ=4, numIterations=1000, **EPS))
    if "sweep" in parts:
        with qps.QuadraticProgramSharedBatch(P, A, Q, L, U) as prob:
            for adaptive in (False, True):
                prob.set_adaptive_rho(adaptive)
                for rho in (0.1, 1.0, 10.0):
                    row = []
                    for on in ([False, True] if have else [False]):
                        if have:
                            prob.set_infeasibility(1e-4 if on else 0, 1e-4 if on else 0)
                        _, flags, infos = prob.solve(ρ=rho, numIterations=2000, **EPS)
                        fl = [int(f) for f in flags]
                        row.append(f"{'on ' if on else 'off'}: column {b} flag {fl[b]} at {infos[b]['iterations']}, longest run {max(i['iterations'] for i in infos)}, "
                                   f"flags {({k: fl.count(k) for k in sorted(set(fl))})}, tLoop {infos[0]['tLoop'] * 1e3:.1f} ms")
                    print(f"dense sweep, {'family rule' if adaptive else 'fixed rho'}, rho {rho}:  " + "   ".join(row), flush=True)


if __name__ == "__main__":
    main()
