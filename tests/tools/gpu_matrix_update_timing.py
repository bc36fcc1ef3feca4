#!/usr/bin/env python
"""What the in-place matrix update of the shared-matrix batches (qps_update_shared_matrices, qps_update_shared_matrices_csc) costs against the only way there
was before: destroy the handle, create a new one on the new matrices, set every option again.  Not a test: it writes a record.

Legs:   dense  c4: n = 1024, m = 2048, 32 columns, fp64                                  (QuadraticProgramSharedBatch, the shape of DESIGN 10c)
        lasso  lasso path numElements = 100, 16 columns, fp64                            (QuadraticProgramSparseSharedBatch, the family of DESIGN 10d)
        cg     GenerateRandomQP(randomQp, 2000, numConstraints = 3000), 16 columns, fp64 (QuadraticProgramCgSharedBatch, the family of DESIGN 10e)
Span:   from "new matrices in hand" to "the first solve has factorised": wall time of the calls that bring the handle to the new matrices plus tSetup of the solve
        that follows (K = 25 iterations, eps 0, rho = 0.1).  The matrices alternate between step 1 and step 2 of tests/matrix_update_cases.py (step_matrices),
        one warm-up round, then REPEATS timed rounds; the median counts.  Options on the handle in both parts: rho scale, family-wide rho rule, warm start "state".
Parts:  update    update_matrices(P, A), solve(reuseFactor=True).  dense also: update_matrices(P) alone (the cached A'A is kept).
        recreate  close(), a new handle on (P, A, Q, L, U), the three options again, solve().  Only calls that exist without the update: --tree DIR imports the package
                  from another checkout (built there), so this part runs on the parent commit.
        compare   --parent DIR: `recreate` on DIR and `update` on this tree in child processes, both times and their ratio per leg.
Nothing is asserted.

    python tests/tools/gpu_matrix_update_timing.py [--parts update,recreate] [--legs dense,lasso,cg] [--tree DIR] [--parent DIR] [--log PATH]
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


def family(qps, leg):
    import numpy as np
    from shared_batch_cases import shared_family
    from sparse_shared_cases import lasso_path
    if leg == "dense":
        return qps.QuadraticProgramSharedBatch, shared_family(1024, 2048, 32), "dense c4: n = 1024, m = 2048, 32 columns"
    if leg == "lasso":
        fam = lasso_path(100, 16)
        return qps.QuadraticProgramSparseSharedBatch, fam, f"sparse lasso path numElements = 100: N = {fam[0].shape[0]}, M = {fam[1].shape[0]}, 16 columns"
    from quadraticprogramsolver_amd.generator import GenerateRandomQP, ProblemClass, make_rng
    P, _, A, _, _ = GenerateRandomQP(ProblemClass.randomQp, 2000, numConstraints=3000, rng=make_rng(77, 1))
    n, m, count = P.shape[0], A.shape[0], 16
    rng = make_rng(78, 1)
    Q, L, U = np.zeros((count, n)), np.zeros((count, m)), np.zeros((count, m))
    for b in range(count):
        Q[b] = rng.standard_normal(n)
        s = A @ (rng.standard_normal(n) / np.sqrt(n))
        L[b] = s - (1 + b) * rng.random(m)
        U[b] = s + (1 + b) * rng.random(m)
    return qps.QuadraticProgramCgSharedBatch, (P, A, Q, L, U), f"CG random: n = {n}, m = {m}, nnz(P) = {P.nnz}, nnz(A) = {A.nnz}, 16 columns"


def options(qps, prob, L, U):
    prob.set_rho_scale(qps.equality_rho_scale(L, U))
    prob.set_adaptive_rho(True)
    prob.set_warm_start("state")


def show(leg, what, spans, setups):
    print(f"   SPAN {leg} {what} {1e3 * statistics.median(spans):.3f} ms from the new matrices to a factorised solve (median of {len(spans)}; "
          f"{1e3 * min(spans):.3f} .. {1e3 * max(spans):.3f}); of it tSetup of the solve {1e3 * statistics.median(setups):.3f} ms", flush=True)


def run(qps, leg, parts):
    from matrix_update_cases import step_matrices
    cls, (P, A, Q, L, U), title = family(qps, leg)
    steps = [step_matrices(P, A, 1), step_matrices(P, A, 2)]
    print(f"== {title}, fp64; K = {K}, {REPEATS} timed rounds after one warm-up", flush=True)
    prob = cls(P, A, Q, L, U)
    options(qps, prob, L, U)
    X, _, _ = prob.solve(**SOLVE)
    if "update" in parts:
        for what, only_p in (("update", False),) + ((("update-P-only", True),) if leg == "dense" else ()):
            spans, setups = [], []
            for r in range(REPEATS + 1):
                P2, A2 = steps[r % 2]
                t0 = time.perf_counter()
                prob.update_matrices(P2, None if only_p else A2)
                t1 = time.perf_counter()
                X, _, infos = prob.solve(X, reuseFactor=True, **SOLVE)
                if r:
                    spans.append(t1 - t0 + infos[0]["tSetup"]); setups.append(infos[0]["tSetup"])
            show(leg, what, spans, setups)
    if "recreate" in parts:
        spans, setups = [], []
        for r in range(REPEATS + 1):
            P2, A2 = steps[r % 2]
            t0 = time.perf_counter()
            prob.close()
            prob = cls(P2, A2, Q, L, U)
            options(qps, prob, L, U)
            t1 = time.perf_counter()
            X, _, infos = prob.solve(X, **SOLVE)
            if r:
                spans.append(t1 - t0 + infos[0]["tSetup"]); setups.append(infos[0]["tSetup"])
        show(leg, "recreate", spans, setups)
    prob.close()


def compare(a):
    me = os.path.abspath(__file__)
    vals = {}
    with open(a.log, "w") as log:
        def emit(s):
            log.write(s + "\n"); log.flush(); print(s, flush=True)
        for leg in a.legs.split(","):
            for label, tree, part in (("parent commit", a.parent, "recreate"), ("this tree", ROOT, "update")):
                cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, me, "--parts", part, "--legs", leg, "--tree", tree]
                out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
                for line in out.stdout.splitlines():
                    emit(f"[{label}] {line}")
                    if " SPAN " in line:
                        w = line.split()
                        vals[(w[1], w[2])] = float(w[3])
                if out.returncode != 0:
                    emit(f"run ({leg}, {part}, {label}) ended with status {out.returncode}: nothing more is started")
                    sys.exit(2)
        emit("-- new matrices to a factorised solve: destroy + create + options on the parent commit | update on this tree | ratio")
        for leg in a.legs.split(","):
            old, new = vals[(leg, "recreate")], vals[(leg, "update")]
            emit(f"   {leg:6s} {old:10.3f} ms | {new:10.3f} ms | {old / new:6.2f} x")
        if ("dense", "update-P-only") in vals:
            emit(f"   dense, P alone: {vals[('dense', 'update-P-only')]:.3f} ms against {vals[('dense', 'update')]:.3f} ms for both matrices")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="update,recreate")
    ap.add_argument("--legs", default="dense,lasso,cg")
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "matrix_update_timing.log"))
    ap.add_argument("--limit", type=int, default=240, help="seconds per child process of --parent")
    a = ap.parse_args()
    if a.parent:
        compare(a)
        return
    sys.path.insert(0, os.path.abspath(a.tree))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.append(ROOT)                                     # the oracle package the case modules read; behind --tree, whose package wins
    import quadraticprogramsolver_amd as qps
    for leg in a.legs.split(","):
        run(qps, leg, a.parts.split(","))


if __name__ == "__main__":
    main()
