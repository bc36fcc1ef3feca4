#!/usr/bin/env python
"""What polishing a whole family at once (qps_polish_shared) costs beside polishing its columns one after the other.

Shapes:  C2 x 16   shared_family(4096, 8192, 16), fp64 (the staged kernel form, one panel)
         C4 x 32   shared_family(1024, 2048, 32), fp64 (the cached form, two panels)
Shared:  the handle's own solve to 1e-4 at rho = 0.1, then polish(X, None, ...) on a copy of that X: `seconds` of the reports (the wall time of the batch's step).
Baseline: the replicated QuadraticProgramBatch of the same family in the same process, solve(polish=True) to 1e-4: it polishes one QP after the other with the
         stand-alone kernels; tPolish summed over the columns.
Both sides take the same numItrPolish, delta, epsMinres and numItrMinres, one warm-up run and the median of three; MINRES iteration counts are per column and
differ between the sides (each polishes its own ADMM state), so the time per MINRES iteration per column is printed beside the totals.  For the shared step that
figure divides the batch's time by the SUM of the columns' iterations; the lockstep count (the iterations of the slowest column, summed over the rounds -- what the
launches follow) is printed too.  Nothing is asserted: the figures are a record.

    python tests/tools/gpu_shared_polish_timing.py [--shapes c2,c4]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
SHAPES = {"c2": (4096, 8192, 16), "c4": (1024, 2048, 32)}
SOLVE = dict(ρ=0.1, ϵAbs=1e-4, ϵRel=1e-4)
POLISH = dict(numItrPolish=3, δ=1e-6, ϵMinres=1e-6, numItrMinres=4000)


def main():
    import numpy as np
    import quadraticprogramsolver_amd as gpu
    from shared_batch_cases import shared_family
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c2,c4")
    args = ap.parse_args()
    for key in args.shapes.split(","):
        n, m, count = SHAPES[key]
        t0 = time.time()
        P, A, Q, L, U = shared_family(n, m, count)
        print(f"{key}: n = {n}, m = {m}, count = {count}, fp64 (generated in {time.time() - t0:.1f} s); polish {POLISH}", flush=True)
        with gpu.QuadraticProgramSharedBatch(P, A, Q, L, U) as fam:
            X0, flags, infos = fam.solve(**SOLVE)
            secs, reps = [], None
            for _ in range(4):
                X = X0.copy()
                reps = fam.polish(X, None, **POLISH)
                secs.append(reps[0]["seconds"])
            secs = secs[1:]
            its = [r["minresIterations"] for r in reps]
            shared = statistics.median(secs)
            print(f"  shared:   ADMM iterations {min(i['iterations'] for i in infos)}..{max(i['iterations'] for i in infos)}, tLoop {infos[0]['tLoop'] * 1e3:.1f} ms; polish "
                  f"{min(secs) * 1e3:.1f} / {shared * 1e3:.1f} / {max(secs) * 1e3:.1f} ms, flags {sorted(set(r['flag'] for r in reps))}, refinements "
                  f"{sorted(set(r['refinements'] for r in reps))}, MINRES per column {min(its)}..{max(its)} (sum {sum(its)}), "
                  f"{shared / sum(its) * 1e6:.2f} us per column-iteration, {shared / max(its) * 1e6:.1f} us per lockstep iteration of the slowest column", flush=True)
        with gpu.QuadraticProgramBatch([(P, Q[b], A, L[b], U[b]) for b in range(count)]) as rep:
            tot, infos = [], None
            for _ in range(4):
                _, flags, infos = rep.solve(polish=True, **SOLVE, **POLISH)
                tot.append(sum(i["tPolish"] for i in infos))
            tot = tot[1:]
            its = [i["polishIterations"] for i in infos]
            base = statistics.median(tot)
            print(f"  baseline: ADMM iterations {min(i['iterations'] for i in infos)}..{max(i['iterations'] for i in infos)}; polish (tPolish summed) "
                  f"{min(tot) * 1e3:.1f} / {base * 1e3:.1f} / {max(tot) * 1e3:.1f} ms, flags {sorted(set(i['polishFlag'] for i in infos))}, MINRES per column "
                  f"{min(its)}..{max(its)} (sum {sum(its)}), {base / max(sum(its), 1) * 1e6:.2f} us per column-iteration", flush=True)
        print(f"  ratio baseline / shared: {base / shared:.2f}x on total polishing time", flush=True)


if __name__ == "__main__":
    main()
