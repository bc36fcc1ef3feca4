#!/usr/bin/env python
"""What the per-constraint rho scale (qps_set_shared_rho_scale) costs per launch and what it buys in iterations, on the shared-matrix batch handles.

Per-kernel times, with and without a scale, in ONE process on ONE handle per shape (the unscaled path is the yardstick: its kernels are untouched):
    dense  c2: n = 4096, m = 8192, 16 columns, fp64      c4: n = 1024, m = 2048, 32 columns, fp64        (the shapes of DESIGN 10c)
    sparse lasso path numElements = 100, 16 columns, fp64                                                (the family of DESIGN 10d)
Protocol: fixed K = 200 iterations (eps 0), numItrConv = 25, rho = 0.1.  Per mode (scalar, equality scale, scalar again): the scale is set or cleared, one
warm-up solve factorises, three unprofiled solves give tLoop per batch-iteration, three profiled solves (qps_set_profiling 2: every launch bracketed) give
the time per launch of every category.  Reported per category: the median of the three and their min .. max.  "scalar again" after the scaled mode shows
the run-to-run spread of the yardstick itself, against which the difference scaled - scalar is to be read.

Iterations to eps = 1e-6 (numIterations = 5000), scalar rho against the equality scale (factor 1e3), per column: shared_family(96, 160, 4) and (200, 330, 4), the c4
family, the lasso path at numElements = 100 and lasso_path(10, 6).  Nothing is asserted: the figures are a record (the iteration ratio depends on the family).

    python tests/tools/gpu_rho_scale_timing.py [--parts dense,sparse,iterations] [--shapes c2,c4]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = {"c2": (4096, 8192, 16), "c4": (1024, 2048, 32)}
K, REPEATS = 200, 3
KW = dict(numIterations=K, ϵAbs=0.0, ϵRel=0.0, ρ=0.1, numItrConv=25)
EPS = dict(numIterations=5000, ϵAbs=1e-6, ϵRel=1e-6, ρ=0.1, numItrConv=25)


def measure(prob, scale, label):
    """-> {category: [us per launch, one per profiled solve]}, [us per batch-iteration, one per unprofiled solve]"""
    prob.set_profiling(0)
    prob.set_rho_scale(scale)
    _, _, infos = prob.solve(**KW)                                   # warm-up: factorises
    setup = infos[0]["tSetup"]
    loops = []
    for _ in range(REPEATS):
        _, _, infos = prob.solve(reuseFactor=True, **KW)
        assert all(i["iterations"] == K for i in infos)
        loops.append(1e6 * infos[0]["tLoop"] / K)
    per = {}
    for _ in range(REPEATS):
        prob.set_profiling(2)                                        # (resets the counters)
        prob.solve(reuseFactor=True, **KW)
        for k in prob.kernel_times():
            if k["launches"] > 0:
                per.setdefault(k["name"], []).append(1e6 * k["seconds"] / k["launches"])
    prob.set_profiling(0)
    print(f"-- {label}: first-solve tSetup {setup * 1e3:.2f} ms; {statistics.median(loops):.1f} us per batch-iteration unprofiled "
          f"(median of {REPEATS}; {min(loops):.1f} .. {max(loops):.1f})")
    for name, v in per.items():
        print(f"   {name:46s} {statistics.median(v):9.2f} us per launch (median of {len(v)}; {min(v):.2f} .. {max(v):.2f})")
    return per, loops


def compare(modes):
    (_, a, la), (_, b, lb), (_, c, lc) = modes
    print("-- difference of medians, us per launch: scaled - scalar | scalar again - scalar (the yardstick's own run-to-run spread)")
    for name in a:
        ma, mb, mc = (statistics.median(x[name]) for x in (a, b, c))
        print(f"   {name:46s} {mb - ma:+8.2f} ({100 * (mb - ma) / ma:+6.2f} %) | {mc - ma:+8.2f} ({100 * (mc - ma) / ma:+6.2f} %)")
    ma, mb, mc = (statistics.median(x) for x in (la, lb, lc))
    print(f"   {'batch-iteration, unprofiled':46s} {mb - ma:+8.2f} ({100 * (mb - ma) / ma:+6.2f} %) | {mc - ma:+8.2f} ({100 * (mc - ma) / ma:+6.2f} %)")


def three_modes(prob, s):
    modes = []
    for label, scale in (("scalar rho", None), ("equality scale x 1e3", s), ("scalar rho again", None)):
        per, loops = measure(prob, scale, label)
        modes.append((label, per, loops))
    compare(modes)


def iterations(prob, s, cols, tag):
    prob.set_rho_scale(None)
    _, fa, ia = prob.solve(**EPS)
    prob.set_rho_scale(s)
    _, fb, ib = prob.solve(**EPS)
    prob.set_rho_scale(None)
    print(f"-- iterations to eps = 1e-6, {tag}, columns {list(cols)}: scalar rho " + " / ".join(f"{ia[b]['iterations']}({int(fa[b])})" for b in cols)
          + " | equality rows x 1e3 " + " / ".join(f"{ib[b]['iterations']}({int(fb[b])})" for b in cols) + "   (flag in parentheses)")
    print(f"   all columns: sum of iterations {sum(i['iterations'] for i in ia)} -> {sum(i['iterations'] for i in ib)}; "
          f"tLoop of the batch {ia[0]['tLoop'] * 1e3:.1f} -> {ib[0]['tLoop'] * 1e3:.1f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="dense,sparse,iterations")
    ap.add_argument("--shapes", default="c2,c4")
    a = ap.parse_args()
    parts = a.parts.split(",")
    import quadraticprogramsolver_amd as qps
    from shared_batch_cases import shared_family
    from sparse_shared_cases import lasso_path
    if "dense" in parts:
        for name in a.shapes.split(","):
            n, m, count = SHAPES[name]
            P, A, Q, L, U = shared_family(n, m, count)
            s = qps.equality_rho_scale(L, U)
            NP, MP = -(-n // 64) * 64, -(-m // 64) * 64
            print(f"== dense {name}: n = {n}, m = {m}, {count} columns, fp64, K = {K}, numItrConv = 25; {int((s > 1).sum())} of {m} rows are equalities; "
                  f"extra device memory with a scale set: {(MP * NP + 3 * MP) * 8 / 2**20:.1f} MiB (diag(sqrt(s)) A and three row vectors)")
            with qps.QuadraticProgramSharedBatch(P, A, Q, L, U) as prob:
                three_modes(prob, s)
                if "iterations" in parts and name == "c4":
                    iterations(prob, s, range(4), f"shared_family({n}, {m}, {count})")
    if "sparse" in parts:
        count = 16
        P, A, Q, L, U = lasso_path(100, count)
        s = qps.equality_rho_scale(L, U)
        print(f"== sparse lasso path numElements = 100: N = {P.shape[0]}, M = {A.shape[0]}, {count} columns, fp64, K = {K}, numItrConv = 25; "
              f"{int((s > 1).sum())} of {A.shape[0]} rows are equalities")
        with qps.QuadraticProgramSparseSharedBatch(P, A, Q, L, U) as prob:
            three_modes(prob, s)
            if "iterations" in parts:
                iterations(prob, s, range(4), "lasso_path(100, 16)")
    if "iterations" in parts:
        P, A, Q, L, U = shared_family(200, 330, 4)
        with qps.QuadraticProgramSharedBatch(P, A, Q, L, U) as prob:
            iterations(prob, qps.equality_rho_scale(L, U), range(4), "shared_family(200, 330, 4)")
        P, A, Q, L, U = shared_family(96, 160, 4)
        with qps.QuadraticProgramSharedBatch(P, A, Q, L, U) as prob:
            iterations(prob, qps.equality_rho_scale(L, U), range(4), "shared_family(96, 160, 4)")
        P, A, Q, L, U = lasso_path(10, 6)
        with qps.QuadraticProgramSparseSharedBatch(P, A, Q, L, U) as prob:
            iterations(prob, qps.equality_rho_scale(L, U), range(6), "lasso_path(10, 6)")


if __name__ == "__main__":
    main()
