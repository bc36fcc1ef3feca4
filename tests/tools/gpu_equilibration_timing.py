#!/usr/bin/env python
"""What the opt-in Ruiz equilibration of the shared-matrix batches (qps_set_shared_equilibration) costs and what it buys.

    dense  c2: n = 4096, m = 8192, 16 columns, fp64      c4: n = 1024, m = 2048, 32 columns, fp64        (the shapes of DESIGN 10c)
    sparse lasso path numElements = 100, 16 columns, fp64                                                (the family of DESIGN 10d)
Parts (rho = 0.1, 10 passes, medians of three with their min .. max):
  set    host wall time of set_equilibration(10) and of set_equilibration(0) on the three handles (the calls return after the device has finished);
  iter   batch-iteration time at a fixed K = 200 (eps = 0): tLoop / K with the option off and on, and the time of one check (profiler category, level 2) beside it;
         --off-only measures the option-off half alone -- the form that also runs in a checkout of the parent commit (--tree), which has no such option;
  eps    iterations to eps = 1e-6 (numIterations = 5000) and tLoop, off and on, on shared_family(96, 160, 4), the same scrambled over three decades and the
         scrambled (200, 330, 4), next to the counts of the numpy restatement.
Nothing is asserted: the figures are a record (the iteration ratio depends on the family).

    python tests/tools/gpu_equilibration_timing.py [--parts set,iter,eps] [--off-only] [--tree DIR]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REPEATS, K, PASSES, RHO = 3, 200, 10, 0.1


def med(v, scale=1.0, fmt=".3f"):
    return f"{statistics.median(v) * scale:{fmt}} ({min(v) * scale:{fmt}} .. {max(v) * scale:{fmt}})"


def handles(qps, names):
    from shared_batch_cases import shared_family
    from sparse_shared_cases import lasso_path
    for name in names:
        if name == "lasso":
            P, A, Q, L, U = lasso_path(100, 16)
            yield f"sparse lasso_path(100, 16): N = {P.shape[0]}, M = {A.shape[0]}, fp64", qps.QuadraticProgramSparseSharedBatch(P, A, Q, L, U)
        else:
            n, m, count = {"c2": (4096, 8192, 16), "c4": (1024, 2048, 32)}[name]
            yield f"dense shared_family({n}, {m}, {count}), fp64", qps.QuadraticProgramSharedBatch(*shared_family(n, m, count))


def part_set(qps, names):
    for tag, prob in handles(qps, names):
        with prob:
            prob.set_equilibration(PASSES); prob.set_equilibration(0)          # warm-up: first launches of the kernels
            on, off = [], []
            for _ in range(REPEATS):
                t0 = time.perf_counter(); prob.set_equilibration(PASSES); t1 = time.perf_counter(); prob.set_equilibration(0); t2 = time.perf_counter()
                on.append(t1 - t0); off.append(t2 - t1)
            print(f"== {tag}: set_equilibration({PASSES}) {med(on, 1e3)} ms, set_equilibration(0) {med(off, 1e3)} ms")


def iteration_times(prob):
    kw = dict(numIterations=K, ϵAbs=0.0, ϵRel=0.0, ρ=RHO)
    prob.solve(**kw)                                                             # warm-up: factorisation, first launches
    loops = [prob.solve(reuseFactor=True, **kw)[2][0]["tLoop"] / K for _ in range(REPEATS)]
    prob.set_profiling(2)
    prob.solve(reuseFactor=True, **kw)
    chk = [k for k in prob.kernel_times() if "check" in k["name"]]
    prob.set_profiling(0)
    return loops, (chk[0]["seconds"] / chk[0]["launches"] if chk else float("nan"))


def part_iter(qps, names, off_only):
    for tag, prob in handles(qps, names):
        with prob:
            loops, chk = iteration_times(prob)
            print(f"== {tag}: option off: {med(loops, 1e6, '.1f')} us per batch iteration, one check {chk * 1e6:.1f} us")
            if off_only:
                continue
            prob.set_equilibration(PASSES)
            loops, chk = iteration_times(prob)
            print(f"   {' ' * len(tag)}  option on:  {med(loops, 1e6, '.1f')} us per batch iteration, one check {chk * 1e6:.1f} us")


def part_eps(qps):
    import equilibration_cases as ec
    kw = dict(numIterations=5000, ϵAbs=1e-6, ϵRel=1e-6, ρ=RHO)
    for key in (("plain", 96, 160, 4), ("scrambled", 96, 160, 4), ("scrambled", 200, 330, 4)):
        P, A, Q, L, U = ec.family(*key)
        with qps.QuadraticProgramSharedBatch(P, A, Q, L, U) as prob:
            for passes in (0, PASSES):
                prob.set_equilibration(passes)
                prob.solve(**kw)
                runs = [prob.solve(**kw) for _ in range(REPEATS)]
                _, flags, infos = runs[-1]
                cpu = ec.run(key, "reduced", passes=passes)["columns"]
                print(f"== {key} passes {passes}: device " + " / ".join(f"{i['iterations']}({int(f)})" for f, i in zip(flags, infos)) + "; restatement "
                      + " / ".join(f"{c['iterations']}({c['convFlag']})" for c in cpu) + f"; tLoop of the batch {med([r[2][0]['tLoop'] for r in runs], 1e3)} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="set,iter,eps")
    ap.add_argument("--shapes", default="c2,c4,lasso")
    ap.add_argument("--off-only", action="store_true")
    ap.add_argument("--tree", default=ROOT, help="root of the checkout whose package is measured (default: this one)")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.abspath(a.tree))
    import quadraticprogramsolver_amd as qps
    print(f"package: {os.path.relpath(os.path.dirname(qps.__file__), ROOT)}")
    names = a.shapes.split(",")
    for part in a.parts.split(","):
        if part == "set":
            part_set(qps, names)
        elif part == "iter":
            part_iter(qps, names, a.off_only)
        elif part == "eps":
            part_eps(qps)


if __name__ == "__main__":
    main()
