"""Bit identity of two builds of libqps_hip.so across every path of the two dense drivers (DenseSolver::solve_once, BatchedDenseSolver::solve_batch) and the
plugin calls of a dense handle.  One dump per build, each in a fresh process; `compare` then demands that every array and every qps_info field except the
times is bitwise equal.  Not a test.

    python tests/tools/gpu_refactor_dump.py dump OUT.npz [--lib PATH/libqps_hip.so]
    python tests/tools/gpu_refactor_dump.py compare A.npz B.npz
    python tests/tools/gpu_refactor_dump.py cycle [--lib PATH] [--cycles N]     # create + solve + destroy at 64 x 128: median microseconds per cycle

The routes are those named in tests/loop_param_cases.py."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

TIMES = ("tSetup", "tLoop", "tRefactor", "tPolish")
RHO = 0.1
BATCH_LOOP_FCTR = 3.0          # 3 x (300, 600), streams 21..23: the CPU oracle switches all three QPs at iteration 26 and QP 2 alone at 101 (numRefactor 1, 1, 2)


def library(argv):
    from quadraticprogramsolver_amd import _lib
    if "--lib" in argv:
        _lib.LIB_PATH = os.path.abspath(argv[argv.index("--lib") + 1])
    _lib.lib()
    import quadraticprogramsolver_amd as q
    return q


def info_array(info):
    keys = sorted(k for k in info if k not in TIMES)
    return keys, np.array([float(info[k]) for k in keys])


def dump(q, path):
    out = {}

    def put(tag, x, zy, info):
        keys, vals = info_array(info)
        out[tag + "/X"], out[tag + "/Z"], out[tag + "/Y"], out[tag + "/info"] = np.array(x), np.array(zy[0]), np.array(zy[1]), vals
        print(f"{tag:40s} " + " ".join(f"{k}={info[k]:g}" for k in ("convFlag", "iterations", "numRefactor", "sweepVariant", "polishFlag")), flush=True)

    def single(tag, shape, dtype="f64", reps=1, **kw):
        n, m = shape
        P, qq, A, l, u = q.GenerateDenseBenchmarkQP(n, m, stream=21, feasible=True)
        base = dict(numIterations=400, ϵAbs=1e-6, ϵRel=1e-6, ρ=RHO)
        base.update(kw)
        with q.QuadraticProgram(P, qq, A, l, u, dtype=dtype) as h:
            for r in range(reps):
                x = np.zeros(n); info = {}
                h.solve(x, info=info, **dict(base, reuseFactor=(r > 0)))
                put(f"{tag}.{dtype}" + (f".resolve{r}" if reps > 1 else ""), x, h.dual(), info)

    for dtype in ("f64", "f32"):
        lv = dict(loopVariant=2) if dtype == "f32" else {}                 # (200, 330) fits the single launch in fp32
        single("reg", (64, 128), dtype)
        single("fused_eager", (200, 330), dtype, numItrConv=2, **lv)
        single("fused_graph", (200, 330), dtype, **lv)
    single("unfused", (200, 330), loopVariant=1)
    single("blocked_sweeps", (1024, 512), trsvBlock=512, numIterations=100)
    single("adaptive_rho", (200, 330), adptΡ=True, fctrΡ=1.0, numItrConv=5, numIterations=60, ϵAbs=0.0, ϵRel=0.0)   # a re-factorisation at every check
    single("adaptive_rho_small", (64, 128), adptΡ=True, fctrΡ=1.0, numItrConv=5, numIterations=60, ϵAbs=0.0, ϵRel=0.0)
    single("reuse_factor", (200, 330), reps=2)
    single("polish", (200, 330), polish=True)
    single("polish_small", (64, 128), polish=True)

    # the plugin calls of a dense handle
    n, m = 200, 330
    P, qq, A, l, u = q.GenerateDenseBenchmarkQP(n, m, stream=21, feasible=True)
    rng = np.random.default_rng(5)
    with q.QuadraticProgram(P, qq, A, l, u) as h:
        x, z, y = rng.standard_normal(n), rng.standard_normal(m), rng.standard_normal(m)
        h.linsys_init(RHO, 1e-6)
        for tag, rho, changed in (("changed0", RHO, False), ("changed1", 0.3, True)):
            xx, zz = np.zeros(n), np.zeros(m)
            h.linsys_solve(x, z, y, rho, 1e-6, changed, xx, zz)
            out[f"linsys_solve.{tag}/xx"], out[f"linsys_solve.{tag}/zz"] = xx, zz
        for op in ("P", "A", "At", "PA", "reduced"):
            out[f"operator_apply.{op}"] = np.array(h.apply(op, z if op == "At" else x, ρ=0.7, σ=0.01))
        print("plugin calls: linsys_init, linsys_solve x 2, operator_apply x 5", flush=True)

    # the batched driver
    def batch(tag, shape, count, reps=1, **kw):
        n, m = shape
        probs = [q.GenerateDenseBenchmarkQP(n, m, stream=21 + b, feasible=True) for b in range(count)]
        if m == 0:
            probs = [(p[0], p[1], np.zeros((0, n)), np.zeros(0), np.zeros(0)) for p in probs]
        X0 = 0.3 * np.random.default_rng(55).standard_normal((count, n))
        base = dict(numIterations=400, ϵAbs=1e-6, ϵRel=1e-6, ρ=RHO)
        base.update(kw)
        with q.QuadraticProgramBatch(probs) as h:
            for r in range(reps):
                X, _, infos = h.solve(X0, **dict(base, reuseFactor=(r > 0)))
                Z, Y = h.dual()
                t = tag + (f".resolve{r}" if reps > 1 else "")
                out[t + "/X"], out[t + "/Z"], out[t + "/Y"] = X, Z, Y
                out[t + "/info"] = np.stack([info_array(i)[1] for i in infos])
                print(f"{t:40s} iterations={[i['iterations'] for i in infos]} numRefactor={[i['numRefactor'] for i in infos]} convFlag={[i['convFlag'] for i in infos]}", flush=True)

    batch("batch_small_adaptive", (64, 128), 3, adptΡ=True, fctrΡ=2.0)
    # lock-step loop.  With fctrΡ = BATCH_LOOP_FCTR all three QPs switch after the first check (at least half: one batched re-factorisation) and one
    # of them once more on its own (fewer than half: that QP alone); numRefactor then reads 1, 1, 2.
    batch("batch_loop_adaptive", (300, 600), 3, adptΡ=True, fctrΡ=BATCH_LOOP_FCTR, numIterations=600)
    batch("batch_loop_reuse_factor", (300, 600), 3, reps=2)
    batch("batch_loop_polish", (300, 600), 3, polish=True)
    batch("batch_small_polish", (64, 128), 3, polish=True)
    batch("batch_fallback_m0", (8, 0), 3, numIterations=50)
    np.savez(path, **out)
    print("wrote", path, len(out), "arrays")


def compare(a, b):
    A, B = np.load(a), np.load(b)
    bad = sorted(set(A.files) ^ set(B.files))
    for k in sorted(set(A.files) & set(B.files)):
        same = A[k].shape == B[k].shape and A[k].tobytes() == B[k].tobytes()
        print(f"{'equal    ' if same else 'DIFFERENT'} {k} {A[k].shape}")
        if not same:
            bad.append(k)
    print(f"{len(A.files)} arrays, {len(bad)} differ or are missing: {bad}")
    return 1 if bad else 0


def cycle(q, cycles):
    """The handle-recycling path the per-device pools exist for: create + solve + destroy at BASELINE config 1's shape."""
    P, qq, A, l, u = q.GenerateDenseBenchmarkQP(64, 128, stream=1, feasible=True)
    ts = []
    for k in range(cycles + 20):
        x = np.zeros(64)
        t0 = time.perf_counter()
        with q.QuadraticProgram(P, qq, A, l, u) as h:
            h.solve(x, numIterations=50000, ϵAbs=1e-7, ϵRel=1e-7, ρ=0.1, adptΡ=True)
        ts.append(time.perf_counter() - t0)
    ts = np.array(ts[20:]) * 1e6
    print(f"create+solve+destroy 64x128: median_us={np.median(ts):.1f} min_us={ts.min():.1f} p90_us={np.percentile(ts, 90):.1f} cycles={cycles}")


if __name__ == "__main__":
    argv = sys.argv[1:]
    if argv and argv[0] == "dump":
        dump(library(argv), argv[1])
    elif argv and argv[0] == "compare":
        sys.exit(compare(argv[1], argv[2]))
    elif argv and argv[0] == "cycle":
        cycle(library(argv), int(argv[argv.index("--cycles") + 1]) if "--cycles" in argv else 300)
    else:
        raise SystemExit(__doc__)
