#!/usr/bin/env python
"""What the family-wide adaptive rho (qps_set_shared_adaptive_rho) costs per switch and what it buys in iterations, on the shared-matrix batch handles.

    dense  c2: n = 4096, m = 8192, 16 columns, fp64      c4: n = 1024, m = 2048, 32 columns, fp64        (the shapes of DESIGN 10c)
    sparse lasso path numElements = 100, 16 columns, fp64                                                (the family of DESIGN 10d)
Protocol: rho = 0.1, eps = 1e-6, numItrConv = 25, fctrRho = 5, numIterations = 5000.  Per handle: one warm-up solve under mode 1 (its tSetup is the first
factorisation of the handle), then three solves under mode 0 and three under mode 1.  Reported: the median of the three and their min .. max.
  cost of one switch = tRefactor / numRefactor of the column that ran longest (host wall time around re-assembly + Cholesky + w, or the numeric L D L'), next to
      the first-solve tSetup of the same handle;
  iterations per column (flag in parentheses) and tLoop of the batch, mode 0 against mode 1, also on shared_family(96, 160, 4) and (200, 330, 4).
Nothing is asserted: the figures are a record (the iteration ratio depends on the family).

    python tests/tools/gpu_family_rho_timing.py [--parts c2,c4,lasso,small]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

REPEATS = 3
KW = dict(numIterations=5000, ϵAbs=1e-6, ϵRel=1e-6, ρ=0.1, numItrConv=25, fctrΡ=5)


def med(v, scale=1.0, fmt=".2f"):
    return f"{statistics.median(v) * scale:{fmt}} ({min(v) * scale:{fmt}} .. {max(v) * scale:{fmt}})"


def record(prob, tag, cols):
    prob.set_adaptive_rho(True)
    _, _, infos = prob.solve(**KW)                                     # warm-up: the handle's first factorisation
    setup = infos[0]["tSetup"]
    out = {}
    for mode in (0, 1):
        prob.set_adaptive_rho(bool(mode))
        loops, per_switch, last = [], [], None
        for _ in range(REPEATS):
            _, flags, infos = prob.solve(**KW)
            loops.append(infos[0]["tLoop"])
            longest = max(infos, key=lambda i: i["iterations"])
            if longest["numRefactor"]:
                per_switch.append(longest["tRefactor"] / longest["numRefactor"])
            last = (flags, infos)
        out[mode] = (loops, per_switch, last)
    prob.set_adaptive_rho(False)
    print(f"== {tag}: first-solve tSetup {setup * 1e3:.2f} ms")
    for mode in (0, 1):
        loops, per_switch, (flags, infos) = out[mode]
        longest = max(infos, key=lambda i: i["iterations"])
        print(f"   mode {mode}: columns {list(cols)}: " + " / ".join(f"{infos[b]['iterations']}({int(flags[b])})" for b in cols)
              + f"; all columns: sum of iterations {sum(i['iterations'] for i in infos)}, flags {sorted(set(int(f) for f in flags))}; "
              f"tLoop of the batch {med(loops, 1e3)} ms")
        if mode:
            print(f"           switches {longest['numRefactor']}, last rho {longest['rhoFinal']:.4g}; one switch {med(per_switch, 1e3, '.3f')} ms "
                  f"(tRefactor / numRefactor), {100 * statistics.median(per_switch) / setup:.0f} % of the first-solve tSetup")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="c2,c4,lasso,small")
    parts = ap.parse_args().parts.split(",")
    import quadraticprogramsolver_amd as qps
    from shared_batch_cases import shared_family
    from sparse_shared_cases import lasso_path
    dense = {"c2": [(4096, 8192, 16)], "c4": [(1024, 2048, 32)], "small": [(96, 160, 4), (200, 330, 4)]}
    for part in parts:
        for n, m, count in dense.get(part, []):
            P, A, Q, L, U = shared_family(n, m, count)
            with qps.QuadraticProgramSharedBatch(P, A, Q, L, U) as prob:
                record(prob, f"dense shared_family({n}, {m}, {count}), fp64", range(4))
        if part == "lasso":
            P, A, Q, L, U = lasso_path(100, 16)
            with qps.QuadraticProgramSparseSharedBatch(P, A, Q, L, U) as prob:
                record(prob, f"sparse lasso_path(100, 16): N = {P.shape[0]}, M = {A.shape[0]}, fp64", range(4))


if __name__ == "__main__":
    main()
