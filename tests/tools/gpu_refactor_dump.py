"""Bit identity of two builds of libqps_hip.so across every path of the two dense drivers (DenseSolver::solve_once, BatchedDenseSolver::solve_batch) and the
plugin calls of a dense handle.  One dump per build, each in a fresh process; `compare` then demands that every array and every qps_info field except the
times is bitwise equal.  Not a test.

    python tests/tools/gpu_refactor_dump.py dump OUT.npz [--lib PATH/libqps_hip.so] [--group dense|sparse|shared]
    python tests/tools/gpu_refactor_dump.py compare A.npz B.npz
    python tests/tools/gpu_refactor_dump.py cycle [--lib PATH] [--cycles N] [--group dense|sparse|shared]   # create + solve + destroy at 64 x 128 (sparse: of a
                                                                                # small CSC and a small sparse ProxQP handle; shared: of one small handle per
                                                                                # kind of the shared-matrix batches): median microseconds per cycle

The routes are those named in tests/loop_param_cases.py, and the whitened route of a reused fp64 solve (handles created under QPS_WHITEN=1, cases of
tests/whitened_cases.py): (200, 330) fresh and reused from x = 0 and from a non-zero start, to eps, polished, under adptΡ (which takes the classic loop) and after
it, and (1100, 2130) with two chunks per row.  For reg, fused_eager, unfused, blocked_sweeps and the whitened reused solves one more solve runs at profiling level 2
and its (category, launches) pairs are dumped as `<route>/launches`: the launch sequence per category is pinned beside the results.  `--group sparse` covers the CSC handle instead -- the CG plugin on every product form, the explicit
reduced matrix, the direct KKT plugin, AUTO, polishing, the plugin calls, the five operators -- and the sparse ProxQP form.  `--group shared` covers the three
handle kinds of the shared-matrix batches (dense Cholesky, sparse KKT L D L', matrix-free CG) on two small families each: fixed 50 iterations, to eps = 1e-6, rho
scale, family rho, equilibration, both warm start modes, certificates, polishing at the end of a solve and as a call, update() + reuseFactor, the three forms of
update_matrices, and every option together.  QPS_GRAPH is read once per process: a
dump started with QPS_GRAPH=0 runs the direct plugin's routes alone, eagerly, under their own tags."""
import contextlib
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

    def launch_sequence(tag, h, x, **kw):
        """One more solve with every launch bracketed: the (category, launches) pairs of kernel_times(), in the order the categories were registered."""
        h.set_profiling(2)
        h.solve(x, **kw)
        out[tag + "/launches"] = np.array([f"{k['name']} x {k['launches']}" for k in h.kernel_times()])
        h.set_profiling(0)
        print(f"{tag:40s} " + "; ".join(out[tag + "/launches"]), flush=True)

    def single(tag, shape, dtype="f64", reps=1, launches=False, **kw):
        n, m = shape
        P, qq, A, l, u = q.GenerateDenseBenchmarkQP(n, m, stream=21, feasible=True)
        base = dict(numIterations=400, ϵAbs=1e-6, ϵRel=1e-6, ρ=RHO)
        base.update(kw)
        with q.QuadraticProgram(P, qq, A, l, u, dtype=dtype) as h:
            for r in range(reps):
                x = np.zeros(n); info = {}
                h.solve(x, info=info, **dict(base, reuseFactor=(r > 0)))
                put(f"{tag}.{dtype}" + (f".resolve{r}" if reps > 1 else ""), x, h.dual(), info)
            if launches:
                launch_sequence(f"{tag}.{dtype}", h, np.zeros(n), **base)

    for dtype in ("f64", "f32"):
        lv = dict(loopVariant=2) if dtype == "f32" else {}                 # (200, 330) fits the single launch in fp32
        single("reg", (64, 128), dtype, launches=True)
        single("fused_eager", (200, 330), dtype, launches=True, numItrConv=2, **lv)
        single("fused_graph", (200, 330), dtype, **lv)
    single("unfused", (200, 330), launches=True, loopVariant=1)
    single("blocked_sweeps", (1024, 512), launches=True, trsvBlock=512, numIterations=100)
    single("adaptive_rho", (200, 330), adptΡ=True, fctrΡ=1.0, numItrConv=5, numIterations=60, ϵAbs=0.0, ϵRel=0.0)   # a re-factorisation at every check
    single("adaptive_rho_small", (64, 128), adptΡ=True, fctrΡ=1.0, numItrConv=5, numIterations=60, ϵAbs=0.0, ϵRel=0.0)
    single("reuse_factor", (200, 330), reps=2)
    single("polish", (200, 330), polish=True)
    single("polish_small", (64, 128), polish=True)

    # the whitened route: fp64 handles created under QPS_WHITEN=1, solves on the cached factor at a fixed rho
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import whitened_cases as W
    from loop_param_cases import api_kw

    def whitened(tag, shape, solves, x0=None, launches=None):
        """One handle, the solves (suffix, keywords) in turn, the first one fresh and the others with reuseFactor, each from x0 (zero when None)."""
        P, qq, A, l, u = W.problem(shape)
        with environment(QPS_WHITEN="1"):                                  # read when the handle is created
            h = q.QuadraticProgram(P, qq, A, l, u)
        with h:
            for r, (sfx, kw) in enumerate(solves):
                x = np.zeros(shape[0]) if x0 is None else np.array(x0); info = {}
                h.solve(x, info=info, reuseFactor=(r > 0), **kw)
                put(f"{tag}.{sfx}", x, h.dual(), info)
            if launches:
                launch_sequence(f"{tag}.reused", h, np.zeros(shape[0]) if x0 is None else np.array(x0), reuseFactor=True, **launches)

    fixed = api_kw(W.fixed_k())                                            # 60 iterations, a check every 10, ϵ = 0
    whitened("whitened", W.SHAPES[0], [("fresh", fixed), ("reused1", fixed), ("reused2", fixed), ("reused_polish", dict(fixed, polish=True)),
                                       ("reused_adaptive_is_classic", dict(fixed, adptΡ=True)), ("reused_after_adaptive", fixed)], launches=fixed)
    whitened("whitened_x0", W.SHAPES[0], [("fresh", fixed), ("reused1", fixed), ("reused2", fixed)], x0=W.start(W.SHAPES[0]))
    whitened("whitened_to_eps", W.SHAPES[0], [("fresh25", api_kw(dict(W.TO_EPS, numIterations=25))), ("reused", api_kw(W.TO_EPS))])
    two = api_kw(W.fixed_k(numIterations=20))                              # (1100, 2130): the smallest shape with more than one chunk per row
    whitened("whitened_two_chunks", W.SHAPES[1], [("fresh", two), ("reused", two)], launches=two)

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


@contextlib.contextmanager
def environment(**kw):
    """The QPS_* variables a handle reads at creation (or a request when it is served), set for the duration of one route."""
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update(kw)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def sparse_qp(n, m, seed, per_row=8.0):
    """P = M'M + I (M with 3 entries per column), A with `per_row` entries per row, bounds of width <= 2 around A x0."""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    M = sp.random(n, n, density=3.0 / n, random_state=rng, data_rvs=rng.standard_normal, format="csc")
    P = (M.T @ M + sp.identity(n)).tocsc()
    A = sp.random(m, n, density=min(1.0, per_row / n), random_state=rng, data_rvs=rng.standard_normal, format="csc") if m else sp.csc_matrix((0, n))
    Ax = A @ rng.standard_normal(n)
    return P, rng.standard_normal(n), A, Ax - rng.random(m), Ax + rng.random(m)


FORMS = {"stream": dict(QPS_SPMV_BLOCKED="0"), "task": dict(QPS_SPMV_BLOCKED="1", QPS_SPMV_SELL="0"), "sell": dict(QPS_SPMV_BLOCKED="1", QPS_SPMV_SELL="1")}


def dump_sparse(q, path):
    from quadraticprogramsolver_amd import _lib
    from quadraticprogramsolver_amd.proxqp import ProxQP, SolveQuadraticProgramProxQP
    import scipy.sparse as sp
    out = {}
    eager = os.environ.get("QPS_GRAPH") == "0"
    small, mid = sparse_qp(600, 400, 1), sparse_qp(16000, 9000, 2)       # mid: three column blocks in fp64, two in fp32

    def solve(tag, prob, linsys, dtype, reps=1, env=None, kinds=None, **kw):
        """One handle, `reps` solves (reuseFactor from the second on; kinds: the linsys constant of each solve when it changes on the handle)."""
        P, qq, A, l, u = prob
        base = dict(numIterations=40, numItrConv=10, ϵAbs=1e-6, ϵRel=1e-6, ρ=RHO)
        base.update(kw)
        with environment(**(env or {})), q.QuadraticProgram(P, qq, A, l, u, linsys=linsys, dtype=dtype) as h:
            for r in range(reps):
                if kinds:
                    h.linsys = kinds[r]
                x = np.zeros(P.shape[0]); info = {}
                t = f"{tag}.{dtype}" + (f".solve{r}" if reps > 1 else "")
                try:
                    h.solve(x, info=info, **dict(base, reuseFactor=(r > 0 and not kinds)))
                except q.QpsError as e:                                          # a refusal is part of the record: its text must not move
                    out[t + "/refused"] = np.frombuffer(str(e).encode(), dtype=np.uint8)
                    print(f"{t:44s} refused: {e}", flush=True)
                    continue
                keys, vals = info_array(info)
                z, y = h.dual()
                out[t + "/X"], out[t + "/Z"], out[t + "/Y"], out[t + "/info"] = x, np.array(z), np.array(y), vals
                print(f"{t:44s} " + " ".join(f"{k}={info[k]:g}" for k in ("convFlag", "iterations", "numRefactor", "cgIterations", "cgExplicit", "polishFlag")), flush=True)

    for dtype in ("f64", "f32"):
        ldl = dict(numIterations=100, numItrConv=25)
        sfx = ".eager" if eager else ""
        solve("ldl" + sfx, small, "ldl", dtype, **ldl)
        solve("ldl_every_iteration_checked" + sfx, small, "ldl", dtype, numIterations=30, numItrConv=1, ϵAbs=0.0, ϵRel=0.0)
        solve("ldl_adaptive" + sfx, small, "ldl", dtype, adptΡ=True, fctrΡ=1.0, numItrConv=5, numIterations=60, ϵAbs=0.0, ϵRel=0.0)
        solve("ldl_reuse_factor" + sfx, small, "ldl", dtype, reps=2, **ldl)
        if eager:
            continue
        nocg = dict(QPS_CG_EXPLICIT="0")
        for form, env in FORMS.items():
            solve("cg_matfree_" + form, mid, "cg", dtype, env=dict(env, **nocg))
            solve("cg_matfree_m0_" + form, sparse_qp(6000, 0, 3), "cg", dtype, env=dict(env, **nocg))
            solve("cg_explicit_adaptive_" + form, small, "cg_explicit", dtype, env=env, adptΡ=True, fctrΡ=1.0, numItrConv=5, numIterations=30, ϵAbs=0.0, ϵRel=0.0)
        for fuse in "01":
            solve("cg_matfree_sell_fusepa" + fuse, mid, "cg", dtype, env=dict(FORMS["sell"], QPS_SPMV_FUSEPA=fuse, **nocg))
        solve("auto_small", small, "cg", dtype, kinds=[_lib.QPS_LINSYS_AUTO])
        solve("auto_mid", mid, "cg", dtype, kinds=[_lib.QPS_LINSYS_AUTO])
        solve("ldl_then_cg_explicit", small, "ldl", dtype, reps=2, kinds=[_lib.QPS_LINSYS_KKT_LDL, _lib.QPS_LINSYS_CG_EXPLICIT])
        solve("polish_cg", small, "cg", dtype, polish=True, numIterations=400, env=nocg)
        solve("polish_ldl", small, "ldl", dtype, polish=True, numIterations=400)

        # the plugin calls and the five operators
        rng = np.random.default_rng(5)
        for linsys, form in (("cg", "stream"), ("cg", "sell"), ("cg_explicit", "stream"), ("cg_explicit", "task"), ("ldl", "stream")):
            P, qq, A, l, u = mid if linsys == "cg" else small
            n, m = P.shape[0], A.shape[0]
            x, z, y = rng.standard_normal(n), rng.standard_normal(m), rng.standard_normal(m)
            with environment(**dict(FORMS[form], **(nocg if linsys == "cg" else {}))), q.QuadraticProgram(P, qq, A, l, u, linsys=linsys, dtype=dtype) as h:
                h.linsys_init(RHO, 1e-6)
                for t, rho, changed in (("changed0", RHO, False), ("changed1", 0.3, True)):
                    xx, zz = np.zeros(n), np.zeros(m)
                    h.linsys_solve(x, z, y, rho, 1e-6, changed, xx, zz)
                    out[f"linsys_solve.{linsys}.{form}.{t}.{dtype}/xx"], out[f"linsys_solve.{linsys}.{form}.{t}.{dtype}/zz"] = xx, zz
                if linsys == "cg":
                    for op in ("P", "A", "At", "PA", "reduced"):
                        out[f"operator_apply.{form}.{op}.{dtype}"] = np.array(h.apply(op, z if op == "At" else x, ρ=0.7, σ=0.01))
        print(f"plugin calls {dtype}: linsys_init, linsys_solve x 2 on five handles; operator_apply x 5 stream and sliced (stacked [P; A])", flush=True)

        # the sliced form staged and lane by lane: a workgroup's share of the rows reaches 1024 only at n = 50 000, m = 100 000 (tests/test_gpu_spmv_operator.py)
        big = sparse_qp(50000, 100000, 4)
        for staged in "10":
            solve("cg_matfree_sell_staged" + staged, big, "cg", dtype, env=dict(FORMS["sell"], QPS_SPMV_STAGED=staged, **nocg), numIterations=4, numItrConv=2)

        # sparse ProxQP
        def proxqp(tag, n, me, mi, explicit_state=False, env=None, **kw):
            r = np.random.default_rng(11)
            P = small[0] if n == 600 else sparse_qp(n, 0, 6)[0]
            A = sp.random(me, n, density=8.0 / n, random_state=r, data_rvs=r.standard_normal, format="csc") if me else sp.csc_matrix((0, n))
            Cm = sp.random(mi, n, density=8.0 / n, random_state=r, data_rvs=r.standard_normal, format="csc") if mi else sp.csc_matrix((0, n))
            x0 = r.standard_normal(n)
            args = (P, r.standard_normal(n), A, A @ x0, Cm, Cm @ x0 + r.random(mi))
            if explicit_state:
                args += (0.1 * r.standard_normal(n), np.zeros(me), np.zeros(mi), np.ones(mi))
            with environment(**(env or {})), ProxQP(*args, dtype=dtype) as pq:
                rep = SolveQuadraticProgramProxQP(pq, **dict(dict(numIterations=60, numItrConv=10), **kw))
                t = f"proxqp_{tag}.{dtype}"
                out[t + "/X"], out[t + "/Y"], out[t + "/Z"], out[t + "/S"] = pq.vX.copy(), pq.vY.copy(), pq.vZ.copy(), pq.vS.copy()
                out[t + "/report"] = np.array([float(rep[k]) for k in sorted(rep)])
                print(f"{t:44s} " + " ".join(f"{k}={rep[k]:g}" for k in sorted(rep)), flush=True)

        proxqp("init_kkt", 600, 100, 300)
        proxqp("set_state", 600, 100, 300, explicit_state=True)
        proxqp("no_equalities", 600, 0, 300)
        proxqp("no_inequalities", 600, 100, 0)
        proxqp("rho_update", 600, 100, 300, ρ=1e-2, numIterations=100)
        proxqp("fixed_rho", 600, 100, 300, adptΡ=False)
        proxqp("gx_from_solve", 600, 100, 300, env=dict(QPS_PROXQP_GX_SOLVE="1"))
    np.savez(path, **out)
    print("wrote", path, len(out), "arrays")


def dump_shared(q, path):
    """The three handle kinds of the shared-matrix batches on the small families of the suite, every option of the family on its own and all together."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import cg_shared_cases as cc
    from matrix_update_cases import step_matrices
    from shared_batch_cases import shared_family
    from sparse_shared_cases import lasso_path, random_family
    out = {}
    families = [("dense_96x160", q.QuadraticProgramSharedBatch, shared_family(96, 160, 6), RHO),
                ("dense_1100x2300", q.QuadraticProgramSharedBatch, shared_family(1100, 2300, 20), RHO),          # two panels
                ("sparse_lasso", q.QuadraticProgramSparseSharedBatch, lasso_path(10, 6), RHO),
                ("sparse_random", q.QuadraticProgramSparseSharedBatch, random_family(20), RHO),
                ("cg_random", q.QuadraticProgramCgSharedBatch, cc.family("random"), cc.RHO["random"]),
                ("cg_banded", q.QuadraticProgramCgSharedBatch, cc.family("banded"), cc.RHO["banded"])]

    def put(tag, h, X, infos, reps=None, cert=False, eq=False):
        Z, Y = h.dual()
        out[tag + "/X"], out[tag + "/Z"], out[tag + "/Y"] = np.array(X), np.array(Z), np.array(Y)
        out[tag + "/info"] = np.stack([info_array(i)[1] for i in infos])
        if reps is not None:
            out[tag + "/polish"] = np.array([[float(r[k]) for k in sorted(r) if k != "seconds"] for r in reps])
        if cert:
            out[tag + "/certDY"], out[tag + "/certDX"] = (np.array(a) for a in h.certificate())
        if eq:
            out[tag + "/eqD"], out[tag + "/eqE"] = (np.array(a) for a in h.equilibration())
        print(f"{tag:44s} iterations={[i['iterations'] for i in infos][:6]} convFlag={[i['convFlag'] for i in infos][:6]} numRefactor={[i['numRefactor'] for i in infos][:3]}",
              flush=True)

    for name, cls, (P, A, Q, L, U), rho in families:
        cg = cls is q.QuadraticProgramCgSharedBatch
        fixed = dict(numIterations=50, numItrConv=25, ϵAbs=0.0, ϵRel=0.0, ρ=rho)
        to_eps = dict(numIterations=2000, numItrConv=5, ϵAbs=1e-6, ϵRel=1e-6, ρ=rho)               # a check every 5 iterations: the columns stop at different checks
        vS = q.equality_rho_scale(L, U, 1e2)
        vS[0] = 10.0                                                                                # not all ones on any family
        P2, A2 = step_matrices(P, A, 1)

        def everything(h):
            h.set_rho_scale(vS)
            h.set_adaptive_rho(True)
            if not cg:
                h.set_equilibration(10)
            h.set_warm_start("state")
            h.set_infeasibility(1e-4, 1e-4)
            h.set_polish(True)

        def route(tag, dtype, prepare=None, second=None, kw=fixed, **flags):
            """One fresh handle: prepare(h), a solve from X = 0; then second(h, X) -> (X0, kw) and a second solve, dumped under .2"""
            t = f"{name}.{tag}.{dtype}"
            with cls(P, A, Q, L, U, dtype=dtype) as h:
                try:
                    if prepare:
                        prepare(h)
                    X, _, infos = h.solve(**kw)
                    put(t, h, X, infos, **flags)
                    if second:
                        X0, kw2 = second(h, X)
                        X, _, infos = h.solve(X0, **kw2)
                        put(t + ".2", h, X, infos, **flags)
                except q.QpsError as e:                                                             # a refusal is part of the record: its text must not move
                    out[t + "/refused"] = np.frombuffer(str(e).encode(), dtype=np.uint8)
                    print(f"{t:44s} refused: {e}", flush=True)

        def all_together(h, X):
            h.update(Q[::-1].copy(), L[::-1].copy(), U[::-1].copy())
            h.update_matrices(P2, A2)
            return X, dict(to_eps, fctrΡ=1.5, reuseFactor=True)

        for dtype in ("f64", "f32"):
            route("fixed50", dtype)
            route("all_options", dtype, everything, all_together, kw=dict(to_eps, fctrΡ=1.5), cert=True, eq=not cg)
        route("to_eps", "f64", kw=to_eps)
        route("rho_scale", "f64", lambda h: h.set_rho_scale(q.equality_rho_scale(L, U)), kw=to_eps)
        route("family_rho", "f64", lambda h: h.set_adaptive_rho(True), kw=dict(to_eps, fctrΡ=1.5))
        if not cg:
            route("equilibration", "f64", lambda h: h.set_equilibration(10), kw=to_eps, eq=True)
        route("warm_state", "f64", lambda h: h.set_warm_start("state"), lambda h, X: (X, to_eps))
        route("warm_ax", "f64", lambda h: h.set_warm_start("ax"), lambda h, X: (X, to_eps))
        route("infeasibility", "f64", lambda h: h.set_infeasibility(1e-4, 1e-4), kw=to_eps, cert=True)
        route("update_reuse", "f64", None, lambda h, X: (h.update(Q[::-1].copy(), L[::-1].copy(), U[::-1].copy()), (None, dict(fixed, reuseFactor=True)))[1])
        for tag, mats in (("update_P", dict(mP=P2)), ("update_A", dict(mA=A2)), ("update_PA", dict(mP=P2, mA=A2))):
            route(tag, "f64", None, lambda h, X, mats=mats: (h.update_matrices(**mats), (None, fixed))[1])
        with cls(P, A, Q, L, U) as h:                                                               # polishing: at the end of a solve, and from the caller's x and y
            h.set_polish(True)
            X, _, infos = h.solve(**to_eps)
            put(f"{name}.polish_on.f64", h, X, infos)
            h.set_polish(False)
            X, _, infos = h.solve(**to_eps)
            Z, Y = h.dual()
            Xp = np.array(X)
            reps = h.polish(Xp, np.array(Y))
            put(f"{name}.polish_call.f64", h, Xp, infos, reps=reps)
    np.savez(path, **out)
    print("wrote", path, len(out), "arrays")


def cycle_shared(q, cycles):
    """create + solve + destroy of one small handle per kind of the shared-matrix batches: median microseconds per cycle"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import cg_shared_cases as cc
    from shared_batch_cases import shared_family
    from sparse_shared_cases import random_family
    for name, cls, fam, rho in (("dense shared 96x160x6", q.QuadraticProgramSharedBatch, shared_family(96, 160, 6), RHO),
                                ("sparse shared random_family(20)", q.QuadraticProgramSparseSharedBatch, random_family(20), RHO),
                                ("cg shared banded_family(20)", q.QuadraticProgramCgSharedBatch, cc.family("banded"), cc.RHO["banded"])):
        ts = []
        for k in range(cycles + 20):
            t0 = time.perf_counter()
            with cls(*fam) as h:
                h.solve(numIterations=50, numItrConv=25, ϵAbs=0.0, ϵRel=0.0, ρ=rho)
            ts.append(time.perf_counter() - t0)
        ts = np.array(ts[20:]) * 1e6
        print(f"create+solve+destroy {name}: median_us={np.median(ts):.1f} min_us={ts.min():.1f} p90_us={np.percentile(ts, 90):.1f} cycles={cycles}", flush=True)


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


def cycle_sparse(q, cycles):
    """create + solve + destroy of a small CSC handle on the CG and on the direct plugin and of a small sparse ProxQP handle (create + init_kkt + solve + destroy);
    then the device bytes one sparse ProxQP handle holds (free memory before and after its creation, pools warm), small and with the column-blocked copies forced."""
    import ctypes
    import scipy.sparse as sp
    from quadraticprogramsolver_amd.proxqp import ProxQP, SolveQuadraticProgramProxQP
    P, qq, A, l, u = sparse_qp(600, 400, 1)
    r = np.random.default_rng(11)

    def proxqp_args(n, me, mi):
        Pn = P if n == 600 else sparse_qp(n, 0, 6)[0]
        Ae = sp.random(me, n, density=8.0 / n, random_state=r, data_rvs=r.standard_normal, format="csc")
        Cm = sp.random(mi, n, density=8.0 / n, random_state=r, data_rvs=r.standard_normal, format="csc")
        x0 = r.standard_normal(n)
        return (Pn, r.standard_normal(n), Ae, Ae @ x0, Cm, Cm @ x0 + r.random(mi))

    pq_args = proxqp_args(600, 100, 300)

    def csc(linsys):
        x = np.zeros(600)
        with q.QuadraticProgram(P, qq, A, l, u, linsys=linsys) as h:
            h.solve(x, numIterations=50, ρ=RHO)

    def proxqp():
        with ProxQP(*pq_args) as pq:
            SolveQuadraticProgramProxQP(pq, numIterations=20, numItrConv=10)

    for name, f in (("csc cg 600x400", lambda: csc("cg")), ("csc ldl 600x400", lambda: csc("ldl")), ("sparse proxqp 600, 100 + 300", proxqp)):
        ts = []
        for k in range(cycles + 20):
            t0 = time.perf_counter(); f(); ts.append(time.perf_counter() - t0)
        ts = np.array(ts[20:]) * 1e6
        print(f"create+solve+destroy {name}: median_us={np.median(ts):.1f} min_us={ts.min():.1f} p90_us={np.percentile(ts, 90):.1f} cycles={cycles}", flush=True)
    hip = ctypes.CDLL("libamdhip64.so")

    def free_bytes():
        a, b = ctypes.c_size_t(), ctypes.c_size_t()
        assert hip.hipMemGetInfo(ctypes.byref(a), ctypes.byref(b)) == 0
        return a.value

    for name, args, env in (("600, 100 + 300", pq_args, {}), ("20000, 2000 + 30000, blocked copies forced", proxqp_args(20000, 2000, 30000), dict(QPS_SPMV_BLOCKED="1"))):
        with environment(**env):
            before = free_bytes()
            with ProxQP(*args, *(np.zeros(args[0].shape[0]), np.zeros(args[2].shape[0]), np.zeros(args[4].shape[0]), np.ones(args[4].shape[0]))):
                held = before - free_bytes()
        print(f"device bytes held by one sparse proxqp handle ({name}): {held}", flush=True)


if __name__ == "__main__":
    argv = sys.argv[1:]
    group = argv[argv.index("--group") + 1] if "--group" in argv else "dense"
    if argv and argv[0] == "dump":
        {"dense": dump, "sparse": dump_sparse, "shared": dump_shared}[group](library(argv), argv[1])
    elif argv and argv[0] == "compare":
        sys.exit(compare(argv[1], argv[2]))
    elif argv and argv[0] == "cycle":
        {"dense": cycle, "sparse": cycle_sparse, "shared": cycle_shared}[group](library(argv), int(argv[argv.index("--cycles") + 1]) if "--cycles" in argv else 300)
    else:
        raise SystemExit(__doc__)
