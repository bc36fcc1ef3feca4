#!/usr/bin/env python
"""Throughput of the matrix-free CG shared-matrix batch (QuadraticProgramCgSharedBatch) against the same columns solved one after the other on stand-alone
QuadraticProgram(..., linsys="cg") handles with QPS_CG_EXPLICIT=0 (the matrix-free operator on both sides).  Not a test: it writes a record.

Families: "random" -- mP and mA of GenerateRandomQP(randomQp, 2000, numConstraints=3000) (sparse CSC, density 0.15: P = M'M is nearly full), columns drawn as
tests/sparse_shared_cases.random_family draws them; "c3" -- the pattern of BASELINE config C3, GenerateSparseBenchmarkQP(50000, 100000, densityA=1e-3), the
same columns.  Protocol: fixed K = 50 ADMM iterations (eps 0), rho = 0.1, epsPcg = 1e-6, at 1, 16 and 64 columns; one warm-up solve, then three timed solves,
the median tLoop counts.  Reported per run: ms per batch, CG iterations per second summed over the columns, the same for the sequential loop, and
ratio = (sum of the columns' stand-alone tLoop) / (the batch's tLoop); one more batch solve runs with every category bracketed (qps_set_profiling 2) for the
per-category times and is not part of the rate.  Both sides run inexact inner solves with the same tolerance, so x agrees at the level of epsPcg only; the
agreement is printed, nothing but "ratio > 1 at 16 and 64 columns" is judged (exit status 1 otherwise).

    python tests/tools/gpu_cg_shared_batch_timing.py [--families random,c3] [--columns 1,16,64] [--baseline-columns N] [--log PATH] [--limit SECONDS]

Every (family, count) run is a child process of its own under `timeout -k 10`; after a child that does not end with status 0 nothing more is started.
--baseline-columns N times only the first N stand-alone handles and scales their sum to `count` (the columns cost nearly the same at fixed K)."""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

K, REPEATS, RHO, EPS_PCG = 50, 3, 0.1, 1e-6


def matrices(name):
    from quadraticprogramsolver_amd.generator import GenerateRandomQP, GenerateSparseBenchmarkQP, ProblemClass, make_rng
    if name == "random":
        P, _, A, _, _ = GenerateRandomQP(ProblemClass.randomQp, 2000, numConstraints=3000, rng=make_rng(77, 1))
    else:
        P, _, A, _, _ = GenerateSparseBenchmarkQP(50000, 100000, densityA=1e-3, seed=77)
    return P, A


def columns(A, n, count):
    """q, l, u per column as random_family draws them: x0 feasible, the bounds widen with the column index."""
    import numpy as np
    from quadraticprogramsolver_amd.generator import make_rng
    m = A.shape[0]
    rng = make_rng(78, 1)
    Q, L, U = np.zeros((count, n)), np.zeros((count, m)), np.zeros((count, m))
    for b in range(count):
        Q[b] = rng.standard_normal(n)
        s = A @ (rng.standard_normal(n) / np.sqrt(n))
        L[b] = s - (1 + b) * rng.random(m)
        U[b] = s + (1 + b) * rng.random(m)
    return Q, L, U


def run(name, count, base_cols):
    import numpy as np
    os.environ["QPS_CG_EXPLICIT"] = "0"                          # read when a stand-alone handle resolves its CG form: matrix-free on both sides
    import quadraticprogramsolver_amd as qps
    P, A = matrices(name)
    n, m = P.shape[0], A.shape[0]
    Q, L, U = columns(A, n, count)
    kw = dict(numIterations=K, ϵAbs=0.0, ϵRel=0.0, ρ=RHO, ϵPcg=EPS_PCG)
    print(f"== {name}: n = {n}, m = {m}, nnz(P) = {P.nnz}, nnz(A) = {A.nnz}, {count} columns, fp64, K = {K}, rho = {RHO}, epsPcg = {EPS_PCG}, "
          f"{REPEATS} timed solves after one warm-up", flush=True)
    with qps.QuadraticProgramCgSharedBatch(P, A, Q, L, U) as prob:
        prob.solve(**kw)
        loops = []
        for _ in range(REPEATS):
            Xs, _, infos = prob.solve(**kw)
            assert all(i["iterations"] == K for i in infos)
            loops.append(infos[0]["tLoop"])
        prob.set_profiling(2)
        prob.solve(**kw)
        kt = prob.kernel_times()
    t_batch = statistics.median(loops)
    cg_batch = sum(i["cgIterations"] for i in infos)
    print(f"shared batch : {t_batch * 1e3:10.2f} ms per batch (median; all: {', '.join(f'{t * 1e3:.2f}' for t in loops)}); {cg_batch} CG iterations over the columns, "
          f"{cg_batch / t_batch:12.0f} CG-it/s")
    for k in kt:
        if k["launches"]:
            per = k["seconds"] / k["launches"]
            print(f"  {k['name']:46s} {k['launches']:6d} samples  {per * 1e6:9.2f} us each  {k['algo_bytes'] / 1e6:9.2f} MB  {k['algo_bytes'] / per / 1e9:8.1f} GB/s")
    cols = min(count, base_cols) if base_cols > 0 else count
    seq, cg_seq, dev = [], 0, 0.0
    for b in range(cols):
        with qps.QuadraticProgram(P, Q[b], A, L[b], U[b], linsys="cg") as one:
            x = np.zeros(n); info = {}
            one.solve(x, info=info, **kw)
            ts = []
            for _ in range(REPEATS):
                x = np.zeros(n)
                one.solve(x, info=info, **kw)
                assert info["iterations"] == K and info["cgExplicit"] == 0
                ts.append(info["tLoop"])
            seq.append(statistics.median(ts))
            cg_seq += info["cgIterations"]
        dev = max(dev, float(np.abs(Xs[b] - x).max() / max(1.0, np.abs(x).max())))
    t_seq = sum(seq) * count / cols
    print(f"sequential   : {t_seq * 1e3:10.2f} ms for {count} columns ({cols} stand-alone handles timed, median of {REPEATS} each); {cg_seq} CG iterations over {cols} columns, "
          f"{cg_seq / sum(seq):12.0f} CG-it/s")
    print(f"ratio sequential / shared = {t_seq / t_batch:.2f}; max rel |x_shared - x_stand-alone| over {cols} columns = {dev:.2e} (inexact inner solves on both sides)")
    return t_seq / t_batch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--families", default="random")
    ap.add_argument("--columns", default="1,16,64")
    ap.add_argument("--baseline-columns", type=int, default=0)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "cg_shared_batch_timing.log"))
    ap.add_argument("--limit", type=int, default=300, help="seconds per (family, count) run")
    ap.add_argument("--run", nargs=2, metavar=("FAMILY", "COUNT"), help="one run in this process (what the parent starts)")
    a = ap.parse_args()
    if a.run:
        ratio = run(a.run[0], int(a.run[1]), a.baseline_columns)
        sys.exit(0 if (int(a.run[1]) < 16 or ratio > 1.0) else 1)
    ok = True
    with open(a.log, "w") as log:
        for fam in a.families.split(","):
            for c in a.columns.split(","):
                cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--run", fam, c, "--baseline-columns", str(a.baseline_columns)]
                res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
                log.write(res.stdout)
                log.flush()
                sys.stdout.write(res.stdout)
                if res.returncode == 1 and "ratio sequential / shared" in res.stdout:
                    ok = False                                   # ran to its end and missed ratio > 1: a finding, the remaining runs are still safe
                    continue
                if res.returncode != 0:
                    msg = f"run ({fam}, {c}) ended with status {res.returncode}: nothing more is started\n"
                    log.write(msg)
                    sys.stdout.write(msg)
                    sys.exit(2)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
