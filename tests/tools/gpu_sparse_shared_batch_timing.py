#!/usr/bin/env python
"""Throughput of the sparse shared-matrix batch (QuadraticProgramSparseSharedBatch) against sequential stand-alone solves on the same family.

Family: the lasso regularisation path of tests/sparse_shared_cases.py at numElements = 100 (N = 10 200 variables, M = 10 100 constraint rows).
Protocol: fixed K = 200 iterations (eps 0), numItrConv = 25, rho = 0.1, at 16, 32 and 64 columns; one warm-up solve, then three timed solves; the
rate is count * K / tLoop in QP-iterations per second (median of the three).  The comparison is `count` sequential solves on stand-alone
QuadraticProgram(linsys="ldl") handles, one per column, in the same process: a rate of count * K / (sum of the columns' tLoop), each handle warmed
up and timed three times like the batch.  A fourth solve of the batch runs with every category bracketed (qps_set_profiling 2) for the per-category
times; it is not part of the rate.  Creation time (analysis + upload) and the first solve's tSetup (numeric factorisation) are reported separately for
both sides.  Nothing is asserted except that both sides agree on x: the figures are a record, not a threshold.

    python tests/tools/gpu_sparse_shared_batch_timing.py [--columns 16,32,64] [--size 100] [--baseline-columns N]

--baseline-columns N times only the first N stand-alone handles (every column costs the same at fixed K) and scales their sum to `count`.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

K, REPEATS = 200, 3
KW = dict(numIterations=K, ϵAbs=0.0, ϵRel=0.0, ρ=0.1, numItrConv=25)


def run(size, count, base_cols):
    import quadraticprogramsolver_amd as qps
    from sparse_shared_cases import lasso_path
    P, A, Q, L, U = lasso_path(size, count)
    n, m = P.shape[0], A.shape[0]
    print(f"== lasso path numElements = {size}: N = {n}, M = {m}, {count} columns, fp64, K = {K}, numItrConv = 25, {REPEATS} timed solves after one warm-up")
    t0 = time.perf_counter()
    prob = qps.QuadraticProgramSparseSharedBatch(P, A, Q, L, U)
    t_create = time.perf_counter() - t0
    with prob:
        Xs, _, infos = prob.solve(**KW)                       # warm-up: the numeric factorisation
        t_setup = infos[0]["tSetup"]
        rates = []
        for _ in range(REPEATS):
            Xs, _, infos = prob.solve(reuseFactor=True, **KW)
            assert all(i["iterations"] == K for i in infos)
            rates.append(count * K / infos[0]["tLoop"])
        t_setup_reused = infos[0]["tSetup"]
        prob.set_profiling(2)
        prob.solve(reuseFactor=True, **KW)
        kt = prob.kernel_times()
    shared = statistics.median(rates)
    print(f"shared batch : {shared:12.0f} QP-it/s (median; all: {', '.join(f'{r:.0f}' for r in rates)}); {1e6 * count / shared:.1f} us per batch-iteration")
    print(f"  creation (analysis + upload) {t_create * 1e3:.1f} ms; first-solve tSetup (numeric factorisation) {t_setup * 1e3:.2f} ms; reused tSetup {t_setup_reused * 1e3:.2f} ms")
    for k in kt:
        per = k["seconds"] / max(k["launches"], 1)
        print(f"  {k['name']:46s} {k['launches']:5d} samples  {per * 1e6:9.2f} us each  {k['algo_bytes'] / 1e6:9.2f} MB  {k['algo_bytes'] / per / 1e9:8.1f} GB/s")
    cols = min(count, base_cols) if base_cols > 0 else count
    loops, creates, setups, dev = [], [], [], 0.0
    for b in range(cols):
        t0 = time.perf_counter()
        one = qps.QuadraticProgram(P, Q[b], A, L[b], U[b], linsys="ldl")
        creates.append(time.perf_counter() - t0)
        with one:
            x = np.zeros(n); info = {}
            one.solve(x, info=info, **KW)                     # warm-up: analysis + numeric factorisation
            setups.append(info["tSetup"])
            ts = []
            for _ in range(REPEATS):
                x = np.zeros(n)
                one.solve(x, info=info, reuseFactor=True, **KW)
                assert info["iterations"] == K
                ts.append(info["tLoop"])
            loops.append(statistics.median(ts))
        dev = max(dev, float(np.abs(Xs[b] - x).max() / max(1.0, np.abs(x).max())))
    seq = cols * K / sum(loops)
    print(f"sequential   : {seq:12.0f} QP-it/s ({cols} stand-alone handles, median of {REPEATS} each); {1e6 * sum(loops) / cols / K:.1f} us per QP-iteration")
    print(f"  creation {1e3 * sum(creates) / cols:.1f} ms per handle; first-solve tSetup (analysis + numeric factorisation) {1e3 * sum(setups) / cols:.1f} ms per handle; "
          f"count x (creation + tSetup) = {1e3 * count * (sum(creates) + sum(setups)) / cols:.0f} ms against {1e3 * (t_create + t_setup):.0f} ms for the batch")
    print(f"ratio shared / sequential = {shared / seq:.2f}")
    # both sides run the same fp64 iteration with the same ordering; the lasso class tolerance of the parity tests (1e-6 relative)
    same = dev <= 1e-6
    print(f"max rel |x_shared - x_stand-alone| over {cols} columns = {dev:.2e} (required <= 1e-6): {'ok' if same else 'THE TWO SIDES DISAGREE'}")
    return same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--columns", default="16,32,64")
    ap.add_argument("--size", type=int, default=100)
    ap.add_argument("--baseline-columns", type=int, default=0)
    a = ap.parse_args()
    ok = True
    for c in a.columns.split(","):
        ok = run(a.size, int(c), a.baseline_columns) and ok
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
