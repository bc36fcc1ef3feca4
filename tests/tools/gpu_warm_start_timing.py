#!/usr/bin/env python
"""What the opt-in warm start of z and y (qps_set_shared_warm_start) buys in iterations and costs per solve, on the shared-matrix batch handles.

Shapes:  dense  c4: n = 1024, m = 2048, 32 columns, fp64      c2: n = 4096, m = 8192, 16 columns, fp64        (the shapes of DESIGN 10c)
         sparse lasso path numElements = 100, 16 columns, fp64                                                (the family of DESIGN 10d)
Parts:
  sequence  a cold solve to eps = 1e-6 (rho = 0.1, numItrConv = 25) and three perturbed re-solves (tests/warm_start_cases.py: step) with update + reuseFactor,
            once in mode 0 (every re-solve starts from the x of the solve before, z = y = 0) and once in mode 1 (from x, z, y): sum of iterations, slowest
            column, tLoop and tSetup per step.
  table     the rows of the case table of tests/warm_start_cases.py on the device, its counts beside the CPU counts of the restatement.
  start     the cost of the start launch itself: qps_set_profiling 2 brackets it -- panel_w in mode 1, the start_z pass (dense) or the CSR product (sparse) in
            mode 2 -- median of three solves.
  mode0     the unprofiled batch-iteration time of mode 0 at fixed K = 200 (eps 0): one warm-up solve, three timed ones.  --tree DIR imports the package from
            another checkout (built there), so the same measurement runs on the parent commit.
  compare   --parent DIR: `mode0` in fresh child processes, parent / this tree / parent again / this tree again, so that the run-to-run spread of either
            build stands beside the difference.  The loop kernels are the same code: anything outside that spread needs an explanation.
Nothing is asserted: the figures are a record (the iteration ratio depends on the family).

    python tests/tools/gpu_warm_start_timing.py [--parts sequence,table,start,mode0] [--shapes c4,c2,lasso] [--tree DIR] [--parent DIR]
"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SHAPES = {"c4": (1024, 2048, 32), "c2": (4096, 8192, 16)}
K, REPEATS = 200, 3
FIXED = dict(ϵAbs=0.0, ϵRel=0.0, ρ=0.1, numItrConv=25)
EPS = dict(numIterations=5000, ϵAbs=1e-6, ϵRel=1e-6, ρ=0.1, numItrConv=25)


def make(qps, name):
    from shared_batch_cases import shared_family
    from sparse_shared_cases import lasso_path
    if name == "lasso":
        fam = lasso_path(100, 16)
        return fam, qps.QuadraticProgramSparseSharedBatch(*fam), f"sparse lasso path numElements = 100: N = {fam[0].shape[0]}, M = {fam[1].shape[0]}, 16 columns, fp64"
    n, m, count = SHAPES[name]
    fam = shared_family(n, m, count)
    return fam, qps.QuadraticProgramSharedBatch(*fam), f"dense {name}: n = {n}, m = {m}, {count} columns, fp64"


def sequence(prob, Q, L, U, mode, steps=3):
    """-> per solve (iterations per column, flags, tLoop, tSetup)"""
    from warm_start_cases import step
    prob.set_warm_start(None)
    prob.update(Q, L, U)
    X, flags, infos = prob.solve(**EPS)
    out = [([i["iterations"] for i in infos], [int(f) for f in flags], infos[0]["tLoop"], infos[0]["tSetup"])]
    prob.set_warm_start(mode)
    for k in range(1, steps + 1):
        prob.update(*step(Q, L, U, k))
        X, flags, infos = prob.solve(X, reuseFactor=True, **EPS)
        out.append(([i["iterations"] for i in infos], [int(f) for f in flags], infos[0]["tLoop"], infos[0]["tSetup"]))
    prob.set_warm_start(None)
    prob.update(Q, L, U)
    return out


def part_sequence(prob, fam):
    _, _, Q, L, U = fam
    runs = {mode: sequence(prob, Q, L, U, mode) for mode in (0, 1)}
    for k in range(4):
        a, b = runs[0][k], runs[1][k]
        print(f"   {'cold solve' if k == 0 else f'step {k}    '}: sum of iterations {sum(a[0]):6d} -> {sum(b[0]):6d}   slowest column {max(a[0]):5d} -> {max(b[0]):5d}   "
              f"tLoop {a[2] * 1e3:8.2f} -> {b[2] * 1e3:8.2f} ms   tSetup {a[3] * 1e3:6.2f} -> {b[3] * 1e3:6.2f} ms   (mode 0 -> mode 1)")
    ta, tb = (sum(r[2] for r in runs[m][1:]) for m in (0, 1))
    print(f"   three re-solves: tLoop {ta * 1e3:.2f} -> {tb * 1e3:.2f} ms; sum of iterations {sum(sum(r[0]) for r in runs[0][1:])} -> {sum(sum(r[0]) for r in runs[1][1:])}")


def part_start(prob, fam):
    _, _, Q, L, U = fam
    prob.set_warm_start(None)
    X, _, _ = prob.solve(numIterations=50, **FIXED)
    for mode, what in (("state", "mode 1"), ("ax", "mode 2")):
        prob.set_warm_start(mode)
        per, setup = [], []
        for _ in range(REPEATS):
            prob.set_profiling(2)
            _, _, infos = prob.solve(X, numIterations=25, reuseFactor=True, **FIXED)
            hit = [k for k in prob.kernel_times() if "warm start" in k["name"] and k["launches"] > 0]
            per += [1e6 * k["seconds"] / k["launches"] for k in hit]
            setup.append(infos[0]["tSetup"] * 1e3)
        prob.set_profiling(0)
        cost = f"{statistics.median(per):.2f} us (median of {len(per)}; {min(per):.2f} .. {max(per):.2f})" if per else "no launch of its own (the first right-hand side reads z and y)"
        print(f"   start launch, {what}: {cost}; tSetup of the solve {statistics.median(setup):.3f} ms")
    prob.set_warm_start(None)


def part_mode0(prob, label):
    prob.set_profiling(0)
    prob.solve(numIterations=K, **FIXED)
    loops = []
    for _ in range(REPEATS):
        _, _, infos = prob.solve(numIterations=K, reuseFactor=True, **FIXED)
        loops.append(1e6 * infos[0]["tLoop"] / K)
    print(f"   MODE0 {label} {statistics.median(loops):.2f} us per batch-iteration, unprofiled, K = {K} (median of {REPEATS}; {min(loops):.2f} .. {max(loops):.2f})")


def part_table(qps):
    import warm_start_cases as wc
    for name, c in wc.CASES.items():
        fam = wc.family(*c["family"])
        cls = qps.QuadraticProgramSparseSharedBatch if c["form"] == "kkt" else qps.QuadraticProgramSharedBatch
        with cls(*fam) as prob:
            runs = {mode: sequence(prob, *fam[2:], mode) for mode in (0, 1)}
        print(f"== case table row {name}: iterations per column, device | CPU restatement")
        for k in range(4):
            show = lambda v: " / ".join(map(str, v)) if len(v) <= 6 else f"sum {sum(v)}, slowest {max(v)}"
            print(f"   {'cold' if k == 0 else f'step {k}'}: x only {show(runs[0][k][0])} | {show(c['x_only'][k])}    x, z, y {show(runs[1][k][0])} | {show(c['iterations'][k])}"
                  f"    {'equal' if runs[0][k][0] == c['x_only'][k] and runs[1][k][0] == c['iterations'][k] else 'DIFFERENT'}")


def compare(a):
    me = os.path.abspath(__file__)
    results = []
    for label, tree in (("parent", a.parent), ("this tree", ROOT), ("parent again", a.parent), ("this tree again", ROOT)):
        out = subprocess.run([sys.executable, me, "--parts", "mode0", "--shapes", a.shapes, "--tree", tree], capture_output=True, text=True, timeout=600)
        if out.returncode != 0:
            sys.stdout.write(out.stdout + out.stderr)
            raise SystemExit(f"mode0 run on {label} failed with status {out.returncode}")
        vals = {}
        for line in out.stdout.splitlines():
            if " MODE0 " in line:
                w = line.split()
                vals[w[1]] = float(w[2])
                print(f"   {label:16s}{line.strip()[5:]}")
        results.append(vals)
    p1, new, p2, new2 = results
    print("-- mode 0, batch-iteration, difference of medians: this tree - parent | parent again - parent (the parent's own run-to-run spread) | this tree again - this tree")
    for s in new:
        print(f"   {s:6s} {new[s] - p1[s]:+8.2f} us ({100 * (new[s] - p1[s]) / p1[s]:+6.2f} %) | {p2[s] - p1[s]:+8.2f} us ({100 * (p2[s] - p1[s]) / p1[s]:+6.2f} %) | "
              f"{new2[s] - new[s]:+8.2f} us ({100 * (new2[s] - new[s]) / new[s]:+6.2f} %)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="sequence,table,start,mode0")
    ap.add_argument("--shapes", default="c4,c2,lasso")
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--parent", default=None)
    a = ap.parse_args()
    parts = a.parts.split(",")
    if a.parent:
        compare(a)
        return
    sys.path.insert(0, os.path.abspath(a.tree))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import quadraticprogramsolver_amd as qps
    for name in a.shapes.split(","):
        if not set(parts) & {"sequence", "start", "mode0"}:
            break
        fam, prob, title = make(qps, name)
        with prob:
            if parts != ["mode0"]:
                print(f"== {title}")
            if "sequence" in parts:
                part_sequence(prob, fam)
            if "start" in parts:
                part_start(prob, fam)
            if "mode0" in parts:
                part_mode0(prob, name)
    if "table" in parts:
        part_table(qps)


if __name__ == "__main__":
    main()
