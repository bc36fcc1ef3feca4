#!/usr/bin/env python
"""What the per-column adaptive rho of the CG shared-matrix batch (qps_set_shared_column_rho) costs per launch and what it buys per column.  Not a test: it
writes a record, nothing is asserted.

Families: "random" -- mP and mA of GenerateRandomQP(randomQp, 2000, numConstraints=3000), columns as tests/sparse_shared_cases.random_family draws them (the
family of DESIGN 10e's table), at 16 and 64 columns, rho = 0.1, fctrRho = 3; "banded" -- tests/cg_shared_cases.banded_family(20), rho = 1, fctrRho = 5.  fp64.

  cost   K = 50 ADMM iterations, eps = 0, epsPcg = 1e-6.  Three solves with every category bracketed (qps_set_profiling 2) per setting; the median of the three
         per-launch times of "CG iteration (4 launches)", "post + update" and "rhs", and the median tLoop of three unprofiled solves: the option off against on
         but never switching (fctrRho = 1e12: the per-column kernels run, no column ever moves).
  ab     the same "off" figures from another built checkout (--other ROOT: the parent commit's, with its own bindings and library), in rounds that alternate
         between the two builds: a parent process runs `cost-off` once per build and round, a fresh process each; the medians of this build should lie inside the
         other build's own min .. max.
  gain   to eps = 1e-6, numIterations = 1000 (--gain-iterations), epsPcg = 1e-6, under the fixed rho, the family rule and the column rule: ADMM iterations per column (min / median
         / max and how many columns end with flag 1), total CG iterations over the columns, tLoop of the batch (median of three).  The batch runs until its
         slowest column: the gain of the column rule is per column.

    python tests/tools/gpu_column_rho_timing.py [--parts cost,gain] [--families random16,random64,banded] [--log PATH]
    python tests/tools/gpu_column_rho_timing.py --parts ab --other OTHER_ROOT [--rounds 3]
"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if "--other" in sys.argv and "cost-off" in sys.argv:                 # a child of part ab on the other build: that checkout's package, this checkout's families
    sys.path.insert(0, os.path.abspath(sys.argv[sys.argv.index("--other") + 1]))
else:
    sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))

REPEATS, K, NEVER = 3, 50, 1e12
CATS = ("CG iteration", "post + update", "rhs")


def family(name):
    import numpy as np
    if name == "banded":
        from cg_shared_cases import banded_family
        return banded_family(20), 1.0, 5.0
    from quadraticprogramsolver_amd.generator import GenerateRandomQP, ProblemClass, make_rng
    count = int(name[len("random"):])
    P, _, A, _, _ = GenerateRandomQP(ProblemClass.randomQp, 2000, numConstraints=3000, rng=make_rng(77, 1))
    n, m = P.shape[0], A.shape[0]
    rng = make_rng(78, 1)
    Q, L, U = np.zeros((count, n)), np.zeros((count, m)), np.zeros((count, m))
    for b in range(count):
        Q[b] = rng.standard_normal(n)
        s = A @ (rng.standard_normal(n) / np.sqrt(n))
        L[b] = s - (1 + b) * rng.random(m)
        U[b] = s + (1 + b) * rng.random(m)
    return (P, A, Q, L, U), 0.1, 3.0


def med(v, scale=1.0, fmt=".2f"):
    return f"{statistics.median(v) * scale:{fmt}} ({min(v) * scale:{fmt}} .. {max(v) * scale:{fmt}})"


def cost_setting(prob, kw):
    """(per-launch microseconds of every category, tLoop) over REPEATS profiled and REPEATS unprofiled solves, after one warm-up."""
    prob.set_profiling(0)
    prob.solve(**kw)
    loops = []
    for _ in range(REPEATS):
        _, _, infos = prob.solve(**kw)
        loops.append(infos[0]["tLoop"])
    per = {c: [] for c in CATS}
    for _ in range(REPEATS):
        prob.set_profiling(2)                                        # setting the level starts the categories over
        prob.solve(**kw)
        for k in prob.kernel_times():
            for c in CATS:
                if k["name"].startswith("cg shared:") and c in k["name"] and k["launches"]:
                    per[c].append(k["seconds"] / k["launches"])
    prob.set_profiling(0)
    return per, loops


def print_cost(tag, per, loops):
    print(f"   {tag:28s} " + "; ".join(f"{c}: {med(per[c], 1e6)} us" for c in CATS if per[c]) + f"; tLoop {med(loops, 1e3)} ms", flush=True)


def cost(qps, name, only_off=False):
    (P, A, Q, L, U), rho, _ = family(name)
    kw = dict(numIterations=K, ϵAbs=0.0, ϵRel=0.0, ρ=rho, ϵPcg=1e-6)
    print(f"== cost, {name}: n = {P.shape[0]}, m = {A.shape[0]}, {Q.shape[0]} columns, fp64, K = {K}, rho = {rho}; median (min .. max) of {REPEATS}", flush=True)
    with qps.QuadraticProgramCgSharedBatch(P, A, Q, L, U) as prob:
        print_cost("off", *cost_setting(prob, kw))
        if only_off:
            return
        prob.set_column_rho()
        per, loops = cost_setting(prob, dict(kw, fctrΡ=NEVER))
        _, _, infos = prob.solve(**dict(kw, fctrΡ=NEVER))
        assert all(i["numRefactor"] == 0 for i in infos)
        print_cost("on, never switching", per, loops)


def gain(qps, name, num_iterations):
    (P, A, Q, L, U), rho, f = family(name)
    kw = dict(numIterations=num_iterations, ϵAbs=1e-6, ϵRel=1e-6, ρ=rho, fctrΡ=f, ϵPcg=1e-6)
    print(f"== gain, {name}: {Q.shape[0]} columns, fp64, to eps = 1e-6 or {num_iterations} iterations, rho = {rho}, fctrRho = {f}, epsPcg = 1e-6; tLoop: median (min .. max) of {REPEATS}", flush=True)
    with qps.QuadraticProgramCgSharedBatch(P, A, Q, L, U) as prob:
        for tag, setup in (("fixed rho", lambda: None), ("family rule", lambda: prob.set_adaptive_rho()), ("column rule", lambda: prob.set_column_rho())):
            prob.set_adaptive_rho(False)
            prob.set_column_rho(False)
            setup()
            prob.solve(**kw)
            loops = []
            for _ in range(REPEATS):
                _, flags, infos = prob.solve(**kw)
                loops.append(infos[0]["tLoop"])
            its = sorted(i["iterations"] for i in infos)
            print(f"   {tag:12s} ADMM iterations per column min / median / max {its[0]} / {statistics.median(its):.0f} / {its[-1]}, sum {sum(its)}, "
                  f"{sum(int(fl) == 1 for fl in flags)} columns at flag 1; CG iterations over the columns {sum(i['cgIterations'] for i in infos)}; switches per column "
                  f"{min(i['numRefactor'] for i in infos)} .. {max(i['numRefactor'] for i in infos)}; rhoFinal {min(i['rhoFinal'] for i in infos):.3g} .. "
                  f"{max(i['rhoFinal'] for i in infos):.3g}; tLoop {med(loops, 1e3)} ms", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="cost,gain")
    ap.add_argument("--families", default="random16,random64,banded")
    ap.add_argument("--other", default=None, help="the root of another built checkout (part ab: the build the off path is compared with)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--gain-iterations", type=int, default=1000)
    ap.add_argument("--limit", type=int, default=240, help="seconds per child process of part ab")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "column_rho_timing.log"))
    a = ap.parse_args()
    parts, fams = a.parts.split(","), a.families.split(",")
    if parts == ["cost-off"]:                                        # a child of part ab: one build, the off path alone
        import quadraticprogramsolver_amd as qps
        for name in fams:
            cost(qps, name, only_off=True)
        return
    with open(a.log, "a" if "ab" in parts and len(parts) == 1 else "w") as log:
        class Tee:
            def write(self, s):
                log.write(s); sys.__stdout__.write(s)

            def flush(self):
                log.flush(); sys.__stdout__.flush()
        sys.stdout = Tee()
        if "ab" in parts:
            print(f"== the off path of this build against the other build (--other): {a.rounds} alternating rounds, a fresh process each", flush=True)
            for r in range(a.rounds):
                for tag, lib in (("other build", a.other), ("this build", None)):
                    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--parts", "cost-off", "--families", a.families]
                    res = subprocess.run(cmd + (["--other", lib] if lib else []), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
                    print(f"-- round {r + 1}, {tag}\n{res.stdout}", end="", flush=True)
                    if res.returncode != 0:
                        print(f"the child ended with status {res.returncode}: nothing more is started", flush=True)
                        sys.stdout = sys.__stdout__
                        sys.exit(2)
        if "cost" in parts or "gain" in parts:
            import quadraticprogramsolver_amd as qps
            for name in fams:
                if "cost" in parts:
                    cost(qps, name)
            for name in fams:
                if "gain" in parts:
                    gain(qps, name, a.gain_iterations)
        sys.stdout.flush()
        sys.stdout = sys.__stdout__                                  # the log closes with this block


if __name__ == "__main__":
    main()
