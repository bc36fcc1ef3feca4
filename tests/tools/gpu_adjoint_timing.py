#!/usr/bin/env python
"""What the adjoint derivatives of a whole family (qps_adjoint_shared) cost beside the polishing step on the same handle, and what the value-gradient kernel does
with the memory system.  Not a test: it writes a record, nothing is asserted.

Points:  c2   shared_family(4096, 8192, 16), fp64, dense handle (the staged kernel form, one panel)
         c4   shared_family(1024, 2048, 32), fp64, dense handle (the cached form, two panels)
         cg   GenerateRandomQP(randomQp, 2000, numConstraints=3000) (4.9 M stored entries in P and A), 16 columns, fp64, CG handle
State:   the handle's own solve (dense: to 1e-4 at rho = 0.1; cg: 50 iterations), y thresholded at 1e-7; g_x ~ N(0, 1).
Whole call:  polish(X, Y) and adjoint(G, X, Y) alternate for --rounds rounds after one warm-up of each, same settings; `seconds` of the reports (the wall time
         of the batch's step) as min / median / max, with the lockstep MINRES count (the slowest column's iterations: what the launches follow).  Both solve
         systems with the same matrix; the right-hand sides differ, so the iteration counts do too, and the time per lockstep iteration is printed beside the totals.
Value kernel (cg): one more adjoint with the profiling brackets on; its category's time, algorithmic bytes (index, row-of-entry index and the 8 B store per
         entry, the four panels once) and the fraction of the achievable HBM rate of DESIGN section 6 (6.29 TB/s).
--polish-only: the polish figures alone, for a run against another build of the library (--lib): the split of polish_panels has to cost nothing.

    python tests/tools/gpu_adjoint_timing.py [--points c2,c4,cg] [--rounds 5] [--polish-only] [--lib PATH/libqps_hip.so] [--tag NAME] [--log PATH]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
SETTINGS = dict(numItrPolish=3, δ=1e-6, ϵMinres=1e-6, numItrMinres=4000)
ACHIEVABLE = 6.29e12


def point(gpu, key):
    import numpy as np
    from gpu_cg_shared_batch_timing import columns, matrices
    from shared_batch_cases import shared_family
    if key == "cg":
        P, A = matrices("random")
        Q, L, U = columns(A, P.shape[0], 16)
        return gpu.QuadraticProgramCgSharedBatch(P, A, Q, L, U), dict(numIterations=50, ϵAbs=0.0, ϵRel=0.0, ρ=0.1), f"nnz(P) {P.nnz}, nnz(A) {A.nnz}, 16 columns"
    n, m, count = {"c2": (4096, 8192, 16), "c4": (1024, 2048, 32)}[key]
    return gpu.QuadraticProgramSharedBatch(*shared_family(n, m, count)), dict(ρ=0.1, ϵAbs=1e-4, ϵRel=1e-4), f"n = {n}, m = {m}, count = {count}"


def fmt(ts):
    return f"{min(ts) * 1e3:.2f} / {statistics.median(ts) * 1e3:.2f} / {max(ts) * 1e3:.2f} ms"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="c2,c4,cg")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--polish-only", action="store_true")
    ap.add_argument("--lib")
    ap.add_argument("--tag", default="this build")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "adjoint_timing.log"))
    a = ap.parse_args()
    import numpy as np
    from quadraticprogramsolver_amd import _lib
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    import quadraticprogramsolver_amd as gpu
    log = open(a.log, "a")

    def say(s):
        print(s, flush=True)
        log.write(s + "\n"); log.flush()

    for key in a.points.split(","):
        t0 = time.time()
        prob, solve, what = point(gpu, key)
        with prob:
            say(f"{key} [{a.tag}]: {what}, fp64 (created in {time.time() - t0:.1f} s); settings {SETTINGS}, {a.rounds} alternating rounds after one warm-up (min / median / max)")
            X, _, _ = prob.solve(**solve)
            Y = prob.dual()[1]
            Y = np.where(np.abs(Y) > 1e-7, Y, 0.0)
            G = np.random.default_rng(3).standard_normal(X.shape)
            tp, ta, rp, ra = [], [], None, None
            for r in range(a.rounds + 1):
                rp = prob.polish(X.copy(), Y, **SETTINGS)
                tp.append(rp[0]["seconds"])
                if not a.polish_only:
                    ra = prob.adjoint(G, X, Y, **SETTINGS)["reports"]
                    ta.append(ra[0]["seconds"])
            lock = lambda reps: max(r["minresIterations"] for r in reps)
            say(f"  polish : {fmt(tp[1:])}; flags {sorted(set(r['flag'] for r in rp))}, lockstep MINRES {lock(rp)}, {statistics.median(tp[1:]) / max(lock(rp), 1) * 1e6:.1f} us per lockstep iteration")
            if a.polish_only:
                continue
            say(f"  adjoint: {fmt(ta[1:])}; flags {sorted(set(r['flag'] for r in ra))}, lockstep MINRES {lock(ra)}, {statistics.median(ta[1:]) / max(lock(ra), 1) * 1e6:.1f} us per lockstep iteration")
            if key != "cg":
                continue
            prob.set_profiling(1)
            for _ in range(3):
                prob.adjoint(G, X, Y, **SETTINGS)
            for k in prob.kernel_times():
                if "adjoint" in k["name"] and k["launches"]:
                    per = k["seconds"] / k["launches"]
                    say(f"  {k['name']}: {k['launches']} samples, {per * 1e6:.2f} us each (both matrices), {k['algo_bytes'] / 1e6:.2f} MB algorithmic, "
                        f"{k['algo_bytes'] / per / 1e9:.1f} GB/s = {k['algo_bytes'] / per / ACHIEVABLE:.3f} of the achievable {ACHIEVABLE / 1e12:.2f} TB/s")


if __name__ == "__main__":
    main()
