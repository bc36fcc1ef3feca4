#!/usr/bin/env python
"""What the values-only update of the sparse shared-matrix batches (qps_update_shared_values) costs against the update that takes the matrices
(qps_update_shared_matrices_csc), on the same handle and the same values.  Not a test: it writes a record.

Legs:   cg        GenerateRandomQP(randomQp, 2000, numConstraints = 3000), 16 columns, fp64   (QuadraticProgramCgSharedBatch; the cg leg of gpu_matrix_update_timing.py)
        lasso     lasso path numElements = 100, 16 columns, fp64                              (QuadraticProgramSparseSharedBatch; its lasso leg)
        lasso-eq  the same with set_equilibration(10): the range test runs, the exponents are kept
Span:   that of gpu_matrix_update_timing.py: from "new values in hand" to "the first solve has factorised" -- wall time of the update call plus tSetup of the solve
        that follows (K = 25 iterations, eps 0, rho = 0.1, reuseFactor).  The values alternate between step 1 and step 2 of tests/matrix_update_cases.py; one
        warm-up round, then REPEATS timed rounds, the median counts, min .. max beside it.  Options on the handle: rho scale, family-wide rho rule, warm start.
Parts:  a  update_matrices(P, A): scipy CSC matrices in hand
        b  update_values(vP, vA): numpy vectors in hand (QPS_MEM_HOST)
        c  update_values(tP, tA): torch device tensors in hand (QPS_MEM_DEVICE)
        The parts alternate inside every round, in one process.  --tree DIR imports the package from another checkout (built there) and runs part a alone: the
        parent commit, whose update_matrices is the yardstick.  --parent DIR: part a on DIR, parts a, b, c on this tree, part a alone on this tree (as the
        parent runs it: back to back, nothing in between), part a on DIR again, in child processes;
        the spans, their ratios and the split of part b (qps_set_profiling categories: staging, validation + verdict read-back, refresh) go to --log.
Nothing is asserted.

    python tests/tools/gpu_value_update_timing.py [--parts a,b,c] [--legs cg,lasso,lasso-eq] [--tree DIR] [--parent DIR] [--log PATH]
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REPEATS, K = 5, 25
SOLVE = dict(numIterations=K, ϵAbs=0.0, ϵRel=0.0, ρ=0.1, numItrConv=25)
NAMES = dict(a="update_matrices", b="update_values-numpy", c="update_values-device")


def show(leg, what, spans, setups):
    print(f"   SPAN {leg} {what} {1e3 * statistics.median(spans):.3f} ms from the new values to a factorised solve (median of {len(spans)}; "
          f"{1e3 * min(spans):.3f} .. {1e3 * max(spans):.3f}); of it tSetup of the solve {1e3 * statistics.median(setups):.3f} ms", flush=True)


def split(prob, update, rounds=3):
    """Stream time of the three profiling categories of update_values per call, over `rounds` profiled calls (events on the handle's stream)."""
    prob.set_profiling(1)
    before = {k["name"]: (k["seconds"], k["launches"]) for k in prob.kernel_times()}
    for r in range(rounds):
        update(r)
    out = []
    for k in prob.kernel_times():
        if k["name"].startswith("shared values:"):
            s0, l0 = before.get(k["name"], (0.0, 0))
            calls = max(1, k["launches"] - l0)
            out.append((k["name"], (k["seconds"] - s0) / calls, k["algo_bytes"]))
    prob.set_profiling(0)
    return out


def run(qps, torch, leg, parts):
    import gpu_matrix_update_timing as mt
    from matrix_update_cases import canonical, step_matrices
    cls, (P, A, Q, L, U), title = mt.family(qps, "lasso" if leg.startswith("lasso") else leg)
    steps = [step_matrices(P, A, 1), step_matrices(P, A, 2)]
    vals = [(canonical(P2).data.copy(), canonical(A2).data.copy()) for P2, A2 in steps]
    print(f"== {leg}: {title}, fp64; nnz(P) = {len(vals[0][0])}, nnz(A) = {len(vals[0][1])}; K = {K}, {REPEATS} timed rounds after one warm-up", flush=True)
    prob = cls(P, A, Q, L, U)
    mt.options(qps, prob, L, U)
    if leg == "lasso-eq":
        prob.set_equilibration(10)
    X, _, _ = prob.solve(**SOLVE)
    dev = [tuple(torch.from_numpy(v).to("cuda:0") for v in pair) for pair in vals] if "c" in parts else None
    if dev:
        torch.cuda.synchronize()
    calls = dict(a=lambda r: prob.update_matrices(*steps[r % 2]), b=lambda r: prob.update_values(*vals[r % 2]), c=lambda r: prob.update_values(*dev[r % 2]))
    spans, setups = {p: [] for p in parts}, {p: [] for p in parts}
    for r in range(REPEATS + 1):
        for p in parts:                                        # the parts alternate inside the round
            t0 = time.perf_counter()
            calls[p](r)
            t1 = time.perf_counter()
            X, _, infos = prob.solve(X, reuseFactor=True, **SOLVE)
            if r:
                spans[p].append(t1 - t0 + infos[0]["tSetup"]); setups[p].append(infos[0]["tSetup"])
    for p in parts:
        show(leg, NAMES[p], spans[p], setups[p])
    for p in [p for p in parts if p in "bc"]:
        for name, sec, nbytes in split(prob, calls[p]):
            print(f"   SPLIT {leg} {NAMES[p]} | {name} | {1e6 * sec:.1f} us per call on the stream | {nbytes / 1e6:.2f} MB counted | "
                  f"{nbytes / max(sec, 1e-12) / 1e9:.1f} GB/s", flush=True)
    prob.close()


def compare(a):
    me = os.path.abspath(__file__)
    vals = {}
    with open(a.log, "w") as log:
        def emit(s):
            log.write(s + "\n"); log.flush(); print(s, flush=True)
        for label, tree, parts in (("parent commit", a.parent, "a"), ("this tree", ROOT, "a,b,c"), ("this tree alone", ROOT, "a"),
                                   ("parent commit again", a.parent, "a")):
            cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, me, "--parts", parts, "--legs", a.legs, "--tree", tree]
            out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            for line in out.stdout.splitlines():
                emit(f"[{label}] {line}")
                if " SPAN " in line:
                    w = line.split()
                    lohi = line.split("(median of")[1].split(";")[1].split(")")[0].strip()
                    vals[(label, w[1], w[2])] = (float(w[3]), lohi)
            if out.returncode != 0:
                emit(f"run ({label}) ended with status {out.returncode}: nothing more is started")
                sys.exit(2)
        emit("-- new values to a factorised solve, median ms (min .. max): update_matrices on the parent commit | again | update_matrices on this tree, alone as "
             "on the parent | alternating with b and c | update_values from numpy | from device tensors | a / b | a / c (a: alternating)")
        for leg in a.legs.split(","):
            g = lambda label, part: vals[(label, leg, NAMES[part])]
            p1, p2, t1 = g("parent commit", "a"), g("parent commit again", "a"), g("this tree alone", "a")
            ta, tb, tc = g("this tree", "a"), g("this tree", "b"), g("this tree", "c")
            emit(f"   {leg:9s} {p1[0]:9.3f} ({p1[1]}) | {p2[0]:9.3f} ({p2[1]}) | {t1[0]:9.3f} ({t1[1]}) | {ta[0]:9.3f} ({ta[1]}) | {tb[0]:9.3f} ({tb[1]}) | "
                 f"{tc[0]:9.3f} ({tc[1]}) | "
                 f"{ta[0] / tb[0]:6.2f} x | {ta[0] / tc[0]:6.2f} x")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="a,b,c")
    ap.add_argument("--legs", default="cg,lasso,lasso-eq")
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "value_update_timing.log"))
    ap.add_argument("--limit", type=int, default=300, help="seconds per child process of --parent")
    a = ap.parse_args()
    if a.parent:
        compare(a)
        return
    parts = a.parts.split(",")
    import torch                                               # before the library, in every process of the comparison: one HIP runtime per process
                                                               # (INTEGRATION.md), and the same one for the parent's part a as for this tree's
    sys.path.insert(0, os.path.abspath(a.tree))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    sys.path.append(ROOT)                                     # the oracle package the case modules read; behind --tree, whose package wins
    import quadraticprogramsolver_amd as qps
    for leg in a.legs.split(","):
        run(qps, torch, leg, parts)


if __name__ == "__main__":
    main()
