#!/usr/bin/env python
"""Throughput of the shared-matrix batch (QuadraticProgramSharedBatch) against the replicated batch (QuadraticProgramBatch) on the same family.

Protocol: fixed K = 200 iterations (eps 0), numItrConv = 25, rho = 0.1; one warm-up solve, then three timed solves of each handle; the rate is
count * K / tLoop in QP-iterations per second (median of the three).  A fourth solve of the shared handle runs with every launch bracketed
(qps_set_profiling 2) for the per-kernel times; it is not part of the rate.

Shapes and required ratios (shared rate / replicated rate):
    c2: n = 4096, m = 8192, 16 columns, fp64   >= 4
    c4: n = 1024, m = 2048, 32 columns, fp64   >= 2
Exits non-zero when a ratio is below its threshold.

    python tests/tools/gpu_shared_batch_timing.py [--shapes c2,c4] [--skip-baseline] [--columns N]

--columns N times the shared batch alone at another column count (how the rate scales past the 32 columns one read of a matrix serves).
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

SHAPES = {"c2": (4096, 8192, 16, 4.0), "c4": (1024, 2048, 32, 2.0)}
K, REPEATS, HBM_PEAK = 200, 3, 8e12
KW = dict(numIterations=K, ϵAbs=0.0, ϵRel=0.0, ρ=0.1, numItrConv=25, reuseFactor=True)


def timed(prob, count):
    prob.solve(**KW)                                   # warm-up (factorises; the timed solves reuse the factor)
    rates, X = [], None
    for _ in range(REPEATS):
        X, flags, infos = prob.solve(**KW)
        assert all(i["iterations"] == K for i in infos)
        rates.append(count * K / infos[0]["tLoop"])
    return rates, X


def run(name, skip_baseline, columns=0):
    import quadraticprogramsolver_amd as qps
    from shared_batch_cases import shared_family
    n, m, count, need = SHAPES[name]
    count = columns or count
    P, A, Q, L, U = shared_family(n, m, count)
    print(f"== {name}: n = {n}, m = {m}, {count} columns, fp64, K = {K}, numItrConv = 25, {REPEATS} timed solves after one warm-up")
    with qps.QuadraticProgramSharedBatch(P, A, Q, L, U) as prob:
        rates, Xs = timed(prob, count)
        prob.set_profiling(2)
        _, _, infos = prob.solve(**KW)
        kt = prob.kernel_times()
    shared = statistics.median(rates)
    print(f"shared     : {shared:12.0f} QP-it/s (median; all: {', '.join(f'{r:.0f}' for r in rates)}); {1e6 * count / shared:.1f} us per batch-iteration")
    loop_bytes = 0.0
    for k in kt:
        per = k["seconds"] / max(k["launches"], 1)
        print(f"  {k['name']:44s} {k['launches']:5d} launches  {per * 1e6:9.2f} us each  {k['algo_bytes'] / 1e6:9.1f} MB  {k['algo_bytes'] / per / 1e9:8.1f} GB/s")
        if "check" not in k["name"]:
            loop_bytes += k["algo_bytes"]
    frac = loop_bytes * shared / count / HBM_PEAK
    print(f"  bytes per iteration (A', tril S, triu S, A and their panels): {loop_bytes / 1e6:.1f} MB -> {loop_bytes * shared / count / 1e12:.3f} TB/s = {frac:.3f} of 8 TB/s")
    if skip_baseline:
        return True
    with qps.QuadraticProgramBatch([(P, Q[b], A, L[b], U[b]) for b in range(count)]) as base:
        brates, Xb = timed(base, count)
    repl = statistics.median(brates)
    print(f"replicated : {repl:12.0f} QP-it/s (median; all: {', '.join(f'{r:.0f}' for r in brates)}); {1e6 * count / repl:.1f} us per batch-iteration")
    dev = float(np.abs(Xs - Xb).max() / max(1.0, np.abs(Xb).max()))
    ratio = shared / repl
    ok = ratio >= need
    print(f"ratio shared / replicated = {ratio:.2f} (required >= {need:g}): {'ok' if ok else 'BELOW THE THRESHOLD'}")
    # both loops run the same fp64 iteration on the same data: the iterate tolerance of the parity tests (1e-9 relative)
    same = dev <= 1e-9
    print(f"max rel |x_shared - x_replicated| = {dev:.2e} (required <= 1e-9): {'ok' if same else 'THE TWO BATCHES DISAGREE'}")
    return ok and same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c2,c4")
    ap.add_argument("--skip-baseline", action="store_true")
    ap.add_argument("--columns", type=int, default=0, help="another column count for the listed shapes (shared batch only: implies --skip-baseline)")
    a = ap.parse_args()
    ok = True
    for name in a.shapes.split(","):
        ok = run(name, a.skip_baseline or a.columns > 0, a.columns) and ok
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
