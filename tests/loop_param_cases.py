"""The case table of tests/test_gpu_loop_params.py (GPU) and tests/test_loop_params_cpu.py (CPU guards): every implementation of the ADMM row update
(SolveQuadraticProgram.jl:56-61) and of the stopping decision (:79-112), the smallest shapes that reach it, and the scalars -- α, σ, an
(ϵAbs, ϵRel) split, numItrConv, fctrΡ -- each one is run with.  Plain importable helper, no device needed.

How each route was confirmed (the handle reports ``sweepVariant`` and ``cgExplicit`` only, so the GPU tests assert those and the rest is read off
the dispatch code):
  reg          qps_dense.hip DenseSolver::solve_once takes the single launch (sweepVariant == 4) when admm_small_supported and loopVariant == 0;
               k_small.hip admm_small picks k_admm_small_reg for NP in {64, 128} with MP / 64 <= 2 (fp64) / 4 (fp32): (64, 128) in both types.
  lds          the same branch with MP / 64 beyond that bound: k_admm_small.  fp64 (64, 130) has MP / 64 = 3 (the (64, 250) draws do not
               reach 1e-3 within 3000 iterations at rho = 0.1); fp32 needs (64, 300), MP / 64 = 5.
  fused_graph  (200, 330) fp64 moves 2.1 MB per iteration, above admm_small_supported's 1.25 MiB: multi-launch loop (sweepVariant != 4), fused
               (loopVariant != 1), replayed as graphs (numItrConv >= 3, NP <= 2048).  In fp32 the shape fits the single launch: loopVariant = 2.
  fused_graph_small   (64, 128) with loopVariant = 2: the same loop at one 64-column block.
  fused_eager  (200, 330) with numItrConv = 2: use_graph needs numItrConv >= 3, so every iteration is enqueued by the host.
  unfused      loopVariant = 1: linear_solve + k_admm_update + the three-product check (LinearSystemSolvers.jl:134-139 order).
  batch_small  qps_dense_batch.hip BatchedDenseSolver::solve_batch: NP = 64, MP = 128 passes admm_small_batch_supported -> k_admm_small_reg_batch, one workgroup per QP.
  batch_lockstep   NP = 192 is neither 64 nor 128: the lock-step loop (k_apass with PassBatch, batched check).
  shared       SharedBatchSolver: EPI 2 / 3 epilogues of k_panel and k_shared_decide; count 18 = a full panel of 16 and a ragged one of 2.  The
               STAGED form of k_panel is the same EPI code in the same template and needs matrices above 32 MiB: left out here, it is covered at
               the default scalars by test_gpu_shared_batch.py::test_staged_kernels_match_the_oracle_and_a_single_column_handle.
  cg_matfree   CSC handle, linsys "cg" with QPS_CG_EXPLICIT=0 (read per request): cgExplicit == 0, host loop with k_admm_update.
  cg_explicit  CSC handle, linsys "cg_explicit": cgExplicit == 1.
  ldl          CSC handle, linsys "ldl": the iterate kernel of k_ldl.hip, plain iterations replayed as a graph."""
import unicodedata
from collections import namedtuple

import numpy as np

from quadraticprogramsolver_amd.generator import GenerateDenseBenchmarkQP, GenerateRandomQP, ProblemClass, make_rng
from shared_batch_cases import shared_family

DEFAULT = (1.6, 1e-6)                                                  # (α, σ) of the reference signature
PARAM_SEQUENCE = (DEFAULT, (1.0, 1e-6), (1.9, 1e-2), (0.5, 1.0), DEFAULT)   # run in this order on ONE handle; the last must repeat the first bit for bit
RHO = 0.1

# kind: dense (QuadraticProgram) / batch (QuadraticProgramBatch) / shared (QuadraticProgramSharedBatch) / csc (QuadraticProgram on CSC, ``linsys``)
# shape32: the shape that reaches the same kernel in fp32 (None: the same); kw / kw32: extra solve() keywords; adpt: adptΡ is supported;
# small: the route reports sweepVariant == 4; env: environment of the request; K: iterations of the fixed-K runs.
Impl = namedtuple("Impl", "key kind shape shape32 count kw kw32 adpt small linsys env K")
STREAM = 21                                                            # GenerateDenseBenchmarkQP / shared_family stream of every dense case


def _impl(key, kind, shape, *, shape32=None, count=1, kw=None, kw32=None, adpt=True, small=False, linsys=None, env=None, K=30):
    return Impl(key, kind, shape, shape32 or shape, count, kw or {}, (kw or {}) if kw32 is None else kw32, adpt, small, linsys, env or {}, K)


IMPLS = [
    _impl("reg", "dense", (64, 128), small=True, K=20),    # K = 20: the fp32 guard needs rel(x) moved by 2e-2 (at K = 25, α = 1.9 moves it by 1.5e-2 only)
    _impl("lds", "dense", (64, 130), shape32=(64, 300), small=True),
    _impl("fused_graph", "dense", (200, 330), kw32=dict(loopVariant=2)),
    _impl("fused_graph_small", "dense", (64, 128), kw=dict(loopVariant=2)),
    _impl("fused_eager", "dense", (200, 330), kw=dict(numItrConv=2), kw32=dict(numItrConv=2, loopVariant=2)),
    _impl("unfused", "dense", (200, 330), kw=dict(loopVariant=1)),
    _impl("batch_small", "batch", (60, 100), count=5),
    _impl("batch_lockstep", "batch", (150, 170), count=3),
    _impl("shared", "shared", (96, 160), count=18, adpt=False),
    _impl("cg_matfree", "csc", None, linsys="cg", env={"QPS_CG_EXPLICIT": "0"}, K=60),
    _impl("cg_explicit", "csc", None, linsys="cg_explicit", K=60),
    _impl("ldl", "csc", None, linsys="ldl"),
]
BY_KEY = {i.key: i for i in IMPLS}
FP32_FIXED_K = ("reg",)                                                # the fixed-K and split-tolerance runs that are repeated in fp32
GRAPH_ROUTES = ("fused_graph", "fused_graph_small", "ldl")             # plain iterations replayed from a captured graph

# fp64: the bounds of test_iterates_match_oracle_all_classes; fp32: those of test_register_resident_single_launch_kernel for that kernel
TOL = {"f64": dict(x=1e-9, z=1e-9, y=1e-8, resPrim=1e-9, resDual=1e-9), "f32": dict(x=2e-3, z=2e-3, y=2e-2, resPrim=2e-3, resDual=2e-2)}

_ASCII_TO_API = {"epsAbs": "ϵAbs", "epsRel": "ϵRel", "rho": "ρ", "sigma": "σ", "alpha": "α", "adptRho": "adptΡ", "fctrRho": "fctrΡ", "epsPcg": "ϵPcg"}


def api_kw(params):
    """Oracle-style keywords (make_params of oracle/c_oracle.py) -> the keywords of the package's solve()."""
    return {api_name(_ASCII_TO_API.get(k, k)): v for k, v in params.items()}


def api_name(name):
    """Python folds identifiers to NFKC (the reference's ϵ, U+03F5, becomes ε, U+03B5): a keyword passed through ** must be spelled that way."""
    return unicodedata.normalize("NFKC", name)


def rel(a, b):
    return np.abs(a - b).max() / max(1.0, np.abs(b).max()) if b.size else 0.0


def shape_of(impl, dtype="f64"):
    return impl.shape32 if dtype == "f32" else impl.shape


_cache = {}


def columns(impl, dtype="f64", to_tolerance=False):
    """The QPs of one case as a list of (mP, vQ, mA, vL, vU, x0): one entry for a single handle, one per QP / column for the batches.
    Batch warm starts are non-zero.  ``to_tolerance``: the data of the runs that stop by a tolerance (the CSC routes change problem).
    Cached; treat as read-only."""
    stream = STREAM
    key = (impl.key, shape_of(impl, dtype) if impl.kind != "csc" else to_tolerance)
    if key in _cache:
        return _cache[key]
    if impl.kind == "csc":
        # The problems are those of test_gpu_ldl.py's ITER_CASES and test_gpu_parity.py's SPARSE_CASES.  The CG plugins stop their inner solve at
        # max(sqrt(eps) ||r0||, ϵPcg) as the reference does, so an iterate is only determined to about 1e-8 of the warm start's residual; the cases
        # below are those on which the oracle's own plugins (matrix-free CG, explicit CG, Cholesky) agree best among themselves:
        #   iterates, cg_*   randomQp n = 200 at K = 60: they agree to 5.5e-10 at (α, σ) = (1.9, 1e-2), 6e-11 or better elsewhere (isotonic n = 600: 5.5e-9)
        #   tolerance, cg_*  huberFitting n = 10 (3010 variables): the orders stop at 225 and 150, the adaptive run refactors once, and the plugins agree
        #                    on rhoFinal to 1.6e-12 (equalityConstrainedQp: 9e-6, a tiny primal residual under the square root of :95)
        #   ldl              randomQp n = 100 / equalityConstrainedQp n = 100, m = 50 (orders stop at 425 and 375): a direct solve, nothing inexact
        if impl.linsys == "ldl":
            pc, n = (ProblemClass.equalityConstrainedQp, 100) if to_tolerance else (ProblemClass.randomQp, 100)
            P, q, A, l, u = GenerateRandomQP(pc, n, numConstraints=50 if to_tolerance else 0, rng=make_rng(1234, 40 + int(pc)))
        elif to_tolerance:
            P, q, A, l, u = GenerateRandomQP(ProblemClass.huberFitting, 10, rng=make_rng(1234, 40 + int(ProblemClass.huberFitting)))
        else:
            P, q, A, l, u = GenerateRandomQP(ProblemClass.randomQp, 200, rng=make_rng(1234, 80 + int(ProblemClass.randomQp)))
        out = [(P, q, A, l, u, np.zeros(P.shape[0]))]
    elif impl.kind == "dense":
        n, m = shape_of(impl, dtype)
        out = [GenerateDenseBenchmarkQP(n, m, stream=stream, feasible=True) + (np.zeros(n),)]
    elif impl.kind == "batch":
        n, m = shape_of(impl, dtype)
        rng = make_rng(55, stream)
        out = [GenerateDenseBenchmarkQP(n, m, stream=stream + b, feasible=True) + (0.3 * rng.standard_normal(n),) for b in range(impl.count)]
    else:
        n, m = shape_of(impl, dtype)
        P, A, Q, L, U = shared_family(n, m, impl.count, stream=stream)
        rng = make_rng(55, stream)
        out = [(P, Q[b], A, L[b], U[b], 0.3 * rng.standard_normal(n)) for b in range(impl.count)]
    _cache[key] = out
    return out


def trivial(col):
    """The exact fixed point on the matrices of ``col``: q = 0, l = -1, u = 1, x0 = 0.  Every iterate is exactly zero in any arithmetic."""
    P, _, A, _, _, _ = col
    n, m = P.shape[0], A.shape[0]
    return (P, np.zeros(n), A, -np.ones(m), np.ones(m), np.zeros(n))


def oracle_kw(impl, to_tolerance=False):
    """What selects the matching plugin of the C oracle.  CG runs drive the inner solve to 1e-12 on both sides, as the existing iterate tests do.
    On the 3010-variable problem of the tolerance runs the oracle's explicit-matrix plugin needs 15 s a run and agrees with its matrix-free one to
    5e-14 in x and 1.6e-12 in rhoFinal: both CG routes are compared with the matrix-free plugin there."""
    from oracle import c_oracle as co
    if impl.kind != "csc":
        return {}
    if impl.linsys == "ldl":
        return dict(linsys=co.KIND_KKT_LDL_SPARSE)
    return dict(linsys=co.KIND_CG_MATFREE if impl.linsys == "cg" or to_tolerance else co.KIND_CG_EXPLICIT, epsPcg=1e-12, numItrPcg=5000)


def solver_kw(impl, dtype="f64"):
    """Extra keywords of the package's solve() for this route (the CG tolerances of ``oracle_kw`` included)."""
    kw = dict(impl.kw32 if dtype == "f32" else impl.kw)
    if impl.kind == "csc" and impl.linsys != "ldl":
        kw.update({api_name("ϵPcg"): 1e-12, "numItrPcg": 5000})
    return kw


def oracle_run(co, impl, col, to_tolerance=False, **params):
    """c_oracle.solve on one column with the case's own numItrConv (fused_eager) and plugin.  ``params`` in the oracle's spelling."""
    P, q, A, l, u, x0 = col
    kw = dict(oracle_kw(impl, to_tolerance))
    if "numItrConv" in impl.kw:
        kw["numItrConv"] = impl.kw["numItrConv"]
    kw.update(params)
    return co.solve(P, q, A, l, u, vX=x0, **kw)


FIXED_K_PERIOD = 10                                                    # divides every K: the last iteration is a check, so the residuals are compared too


def fixed_k(impl, alpha, sigma):
    nc = impl.kw.get("numItrConv", FIXED_K_PERIOD)
    assert impl.K % nc == 0
    return dict(numIterations=impl.K, numItrConv=nc, epsAbs=0.0, epsRel=0.0, rho=RHO, alpha=alpha, sigma=sigma)


# ---------------------------------------------------------------------------------------------------------------------
# Split tolerances.  Every fp64 implementation runs both orders at a fixed ρ = 0.1; those with adptΡ also (1e-3, 1e-9) with fctrΡ = 2 and
# numItrConv = 7 (fused_eager keeps its 2: a period of 3 or more would turn it into fused_graph).
# Each run asserts the oracle's stopping iteration, so tests/test_loop_params_cpu.py demands margin on both sides of the stop; a case that
# sits on a knife edge there gets other data, it is never dropped (stream 21 passes on every route).
# ---------------------------------------------------------------------------------------------------------------------
SPLIT_PAIRS = ((1e-3, 1e-9), (1e-9, 1e-3))


def split_runs(impl):
    """[(tag, oracle-style params)] of the split-tolerance runs of one implementation."""
    runs = [(f"fixed_rho_{a:g}_{r:g}", dict(numIterations=3000, epsAbs=a, epsRel=r, rho=RHO)) for a, r in SPLIT_PAIRS]
    if impl.adpt:
        runs.append(("adaptive_rho_0.001_1e-09", dict(numIterations=3000, epsAbs=1e-3, epsRel=1e-9, rho=RHO, adptRho=True, fctrRho=2.0, numItrConv=impl.kw.get("numItrConv", 7))))
    return runs


# ---------------------------------------------------------------------------------------------------------------------
# Check period and graph run lengths: numIterations = 37 with numItrConv in {3, 4, 7} on the graph-replay routes.  Once to ϵ = 0 (37 iterations:
# the tail after the last check is shorter than a period) and once to PERIOD_EPS, at which the oracle stops at a check that is not the last.
# ---------------------------------------------------------------------------------------------------------------------
PERIODS = (3, 4, 7)
PERIOD_ITERATIONS = 37
# (impl key, numItrConv) -> ϵAbs = ϵRel of the early-stopping run; the oracle then stops at iteration 21, 20, 21 / 18, 20, 21 / 18, 16, 21
PERIOD_EPS = {("fused_graph", 3): 0.15, ("fused_graph", 4): 0.15, ("fused_graph", 7): 0.15,
              ("fused_graph_small", 3): 0.1, ("fused_graph_small", 4): 0.1, ("fused_graph_small", 7): 0.1,
              ("ldl", 3): 0.02, ("ldl", 4): 0.03, ("ldl", 7): 0.02}


def period_runs(impl):
    out = []
    for nc in PERIODS:
        out.append((f"numItrConv{nc}_eps0", dict(numIterations=PERIOD_ITERATIONS, numItrConv=nc, epsAbs=0.0, epsRel=0.0, rho=RHO)))
        e = PERIOD_EPS[(impl.key, nc)]
        out.append((f"numItrConv{nc}_stops_early", dict(numIterations=PERIOD_ITERATIONS, numItrConv=nc, epsAbs=e, epsRel=e, rho=RHO)))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# The stall stop and ϵAdmm = min(ϵAbs, ϵRel) * 1e-2 (:34).  On the runs above convPrimDual fires long before the step |x - xp| falls to 1e-2 of even
# the LARGER tolerance, so they cannot tell min from max.  Here every row is an equality l = u = t with more rows than variables: no x satisfies
# them, the residuals stay O(1), convPrimDual never fires and the run ends by convAdmm when the step reaches ϵAdmm.  With (1e-2, 1e-4) that is
# 1e-6; a max for the min would stop at 1e-4, hundreds of iterations earlier (the oracle with both tolerances at 1e-2 shows where).
# The CSC routes run the ``reg`` problem as sparse matrices.
# ---------------------------------------------------------------------------------------------------------------------
STALL = dict(numIterations=8000, epsAbs=1e-2, epsRel=1e-4, rho=RHO)


def stall_columns(impl):
    key = (impl.key, "stall")
    if key not in _cache:
        import scipy.sparse as sp
        out = []
        for b, (P, q, A, _, _, x0) in enumerate(columns(BY_KEY["reg"] if impl.kind == "csc" else impl)):
            t = 0.5 * make_rng(56, b).standard_normal(A.shape[0])
            if impl.kind == "csc":
                P, A = sp.csc_matrix(P), sp.csc_matrix(A)
            out.append((P, q, A, t, t.copy(), x0))
        _cache[key] = out
    return _cache[key]
