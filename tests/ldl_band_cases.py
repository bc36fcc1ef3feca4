"""The case table of tests/test_gpu_ldl_bands.py (GPU) and tests/test_ldl_bands_cpu.py (CPU guards): small KKT matrices that between them reach every
lane-group form of the two scalar triangular sweeps of k_ldl.hip, k_ldl_fwd<T, LPR> and k_ldl_bwd<T, LPR> with LPR in {1, 4, 16, 64, 256}, the signed
dense tail and a K-split Schur complement with a ragged last slice.  Plain importable helper, no device needed.

The dispatch.  pick_lpr (ldl_symbolic.h) picks LPR per elimination-tree level from the level's mean row (forward, CSR) or column (backward, CSC) length
and once more for the tail rows: <= 2 -> 1, <= 12 -> 4, <= 96 -> 16, <= 1024 (or more than 2048 rows) -> 64, else 256.  Level 0 has no forward launch.  A
launch packs 256 / LPR rows into a workgroup; a level whose row count is no multiple of that is "ragged" (the `valid` mask of the kernel is live).  LPR = 256
is one workgroup per row, so it has no ragged form.  ``pick_lpr`` / ``forms`` below restate the rule; the CPU guards hold the restatement against the
library's own pick_lpr and every case's claim (``shape`` / ``fwd`` / ``bwd`` / ``tail`` of CASES) against ldl_analyze in the host-only build.

The patterns.  dense(n1, m1): fully dense n1 x n1 P and m1 x n1 A; blocks(k, n1, m1): a block-diagonal KKT of k such blocks (every level has k rows);
banded(n, bw): _banded_problem of tests/test_gpu_ldl.py.  Minimum degree eliminates the constraint rows of a dense pattern first as one wide level,
after which row and column lengths walk through all the thresholds.  Values: per block P = M'M / n1 + I, A = G / sqrt(n1), M and G standard normal from
make_rng(2024, case index); cond(K) stays below ~1e3 for rho in {0.3, 40, 1e-3}, so fp32 can be held to ~1e-5 rather than the 5e-2 of the generator's
classes with zero blocks in P.  The QPS_LDL_MAX_TAIL / QPS_LDL_MIN_LEVEL of a case are read when the handle analyses its KKT matrix.

The runs.  Per case the plugin pair in isolation (LinearSystemSolvers.jl:16-44), STEPS = (changedRho, rho) four times with fresh x, z ~ N(0, 1) and
y = rho w, w ~ N(0, 1), from make_rng(78, case index): K [x~; nu] = [sigma x - q; z - y / rho], z~ = z + (nu - y) / rho.  Reference: ``reference_solve``, a dense fp64 LU (sparse LU
for the sparse patterns) with one step of iterative refinement.  fp64 bound 1e-9 relative (``rel`` of test_gpu_ldl.py).  fp32 bound per case and step:
FP32_MARGIN x the error of ``emulate_f32`` -- L D L' without pivoting and the two substitutions in numpy.float32, sequential sums, in the permutation the
analysis returns -- recorded in EMU_F32.  The margin is over the reference's own fp32 error: the device sums lane-strided partial sums (4 or 2
accumulators per lane, then a tree) and contracts to FMA where the emulation sums sequentially.  Every recorded figure must stay <= EMU_LIMIT so that the
bound can still tell a dropped partial sum from rounding (CPU guard).  That limit is why y scales with rho: nu = y + rho (A x~ - z), so with y ~ N(0, 1) at
rho = 1e-3 the post-step (nu - y) / rho cancels three digits of nu in fp32 whichever kernel ran, and the emulation's own z~ error reached 7.9e-4 on
banded2000x8, 5.5e-4 on banded600x5 and 1.2e-4 on blocks37x12x20; with y = rho w the largest figure of the table is 4.8e-6.  EMU_F32 is recorded with
    PYTHONPATH=. python tests/ldl_band_cases.py
(from the repository root), which prints the forms of every case, the same enumeration over PAIR_CASES of tests/test_gpu_ldl.py and the dictionary.

dense(1100, 1300) of the first enumeration is not a case: 2.9 M entries of L, and every coverage condition holds without it.  dense300x30-tail64 is there
for the 64-lane form on the tail rows, which no other small case reaches.

Measured on an MI355X (printed before every assertion, run with -s).  fp64: x~ and z~ within 3.2e-15 over all 32 solves.  fp32: the largest error of a
case is 0.30 ... 1.02 x its emulation's own error (blocks37x12x20 x~ 0.98, banded600x5 z~ 1.02), at most 0.127 of a bound; the 8 x margin was never
needed.  Panel runs: x 2.5e-15, z 1.1e-14, y 6.3e-15, resPrim 2.7e-15, resDual 3.3e-15.  23 tests in 2.9 s.  Two deliberate breaks, each run once in a
throw-away build: group_sum<T, 256> without its fourth wave sum fails exactly the three cases with a 256-lane launch, in both types; k_ldl_bwd stepping
3 LPR instead of 2 LPR at LPR = 4 fails exactly the five cases with a bwd 4 level, in both types."""
import ctypes as C
import functools
import math
from collections import namedtuple

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from quadraticprogramsolver_amd.generator import make_rng

LPRS = (1, 4, 16, 64, 256)
SPRS = (1, 4, 16)
SIGMA = 1e-6
STEPS = ((False, 0.3), (True, 40.0), (False, 40.0), (True, 1e-3))      # (changedRho, rho); linsys_init runs at rho = 0.3
TOL_F64 = 1e-9
FP32_MARGIN = 8.0
EMU_LIMIT = 1e-4
DEFAULT_LIMITS = (8192, 64, 4096)                                      # QPS_LDL_MAX_TAIL, QPS_LDL_MIN_LEVEL, QPS_LDL_MAX_LEVELS when unset


# ---------------------------------------------------------------------------------------------------------------------
# The dispatch of k_ldl.hip, restated
# ---------------------------------------------------------------------------------------------------------------------
def pick_lpr(nnz, rows):
    if rows <= 0:
        return 1
    avg = float(nnz) / rows
    return 1 if avg <= 2.0 else 4 if avg <= 12.0 else 16 if avg <= 96.0 else 64 if (avg <= 1024.0 or rows > 2048) else 256


def pick_panel_spr(nnz, rows):
    """panel_strips.h: strips per (row, panel) of the panel sweeps of the shared-matrix batch."""
    if rows <= 0:
        return 1
    avg = float(nnz) / rows
    return 1 if avg <= 8.0 else 4 if avg <= 64.0 else 16


Launch = namedtuple("Launch", "level lpr rows ragged spr")             # level -1: the tail rows


def forms(level_ptr, rp_at, cp_at, Ns, N, tail_nnz):
    """What SparseLdlImpl launches per solve: {"fwd": [Launch per level >= 1], "bwd": [Launch per level], "tail": Launch or None}.  rp_at / cp_at: rp / cp
    of the factor at the level boundaries; tail_nnz = rp[N] - rp[Ns]."""
    def launch(level, nnz, rows):
        lpr = pick_lpr(nnz, rows)
        return Launch(level, lpr, rows, rows % (256 // lpr) != 0, pick_panel_spr(nnz, rows))
    L = len(level_ptr) - 1
    rows = [int(level_ptr[l + 1] - level_ptr[l]) for l in range(L)]
    assert all(r > 0 for r in rows) and (L == 0 or level_ptr[L] == Ns)
    return {"fwd": [launch(l, int(rp_at[l + 1] - rp_at[l]), rows[l]) for l in range(1, L)],
            "bwd": [launch(l, int(cp_at[l + 1] - cp_at[l]), rows[l]) for l in range(L)],
            "tail": launch(-1, int(tail_nnz), N - Ns) if N > Ns else None}


def schur_slices(ldt, ntc):
    """The K split of the tail's Schur complement (SparseLdlImpl's constructor): (KC, slices, columns of the last slice) for ntc sparse columns that reach
    into a tail of leading dimension ldt; (0, 0, 0) without a Schur complement."""
    if ldt <= 0 or ntc <= 0:
        return 0, 0, 0
    tiles = (ldt // 64) * (ldt // 64 + 1) // 2
    nsplit = min(256, max(1, 768 // tiles))
    KC = max(64, (-(-ntc // nsplit) + 15) // 16 * 16)
    KC = min(KC, 4096)
    nsplit = max(1, -(-ntc // KC))
    return KC, nsplit, ntc - (nsplit - 1) * KC


# ---------------------------------------------------------------------------------------------------------------------
# The host-only build of the analysis (tests/capi/layout_shim.cpp)
# ---------------------------------------------------------------------------------------------------------------------
def _shim():
    import host_shim
    L = host_shim.rules()
    p64 = C.POINTER(C.c_int64)
    L.lt_ldl_level_shape.restype = C.c_int
    L.lt_ldl_level_shape.argtypes = [C.c_int, C.c_int, p64, p64, p64, p64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, p64, p64, p64, p64]
    L.lt_ldl_analyze.restype = C.c_int
    L.lt_ldl_analyze.argtypes = [C.c_int, C.c_int, p64, p64, p64, p64, C.c_int, C.c_int, C.c_int, C.c_int, p64, p64]
    L.lt_pick_lpr.restype = C.c_int
    L.lt_pick_lpr.argtypes = [C.c_int64, C.c_int]
    return L


def library_pick_lpr(nnz, rows):
    return _shim().lt_pick_lpr(int(nnz), int(rows))


def _csc_index(M):
    M = sp.csc_matrix(M)
    M.sort_indices()
    return np.ascontiguousarray(M.indptr, dtype=np.int64), np.ascontiguousarray(M.indices, dtype=np.int64)


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


Shape = namedtuple("Shape", "N Ns Nt ldt levels pos neg ntc forms")


def analyze(P, A, limits=DEFAULT_LIMITS):
    """ldl_analyze of the host-only build on the patterns of P and A under (max_tail, min_level, max_levels): (Shape, perm) with perm[new] = old."""
    n, m = P.shape[0], A.shape[0]
    Pcp, Pri = _csc_index(P)
    Acp, Ari = _csc_index(A)
    cap = n + m + 2
    lp, rpa, cpa = (np.zeros(cap, dtype=np.int64) for _ in range(3))
    misc, perm, rep = np.zeros(8, dtype=np.int64), np.zeros(n + m, dtype=np.int64), np.zeros(8, dtype=np.int64)
    L = _shim().lt_ldl_level_shape(n, m, _ip(Pcp), _ip(Pri), _ip(Acp), _ip(Ari), 0, *limits, cap, _ip(lp), _ip(rpa), _ip(cpa), _ip(misc))
    assert L >= 0, L
    rc = _shim().lt_ldl_analyze(n, m, _ip(Pcp), _ip(Pri), _ip(Acp), _ip(Ari), 0, *limits, _ip(perm), _ip(rep))
    assert rc == 0 and (rep[0], rep[1], rep[2], rep[3]) == (misc[0], misc[1], misc[2], L)
    N, Ns, Nt, ldt, tail_nnz, pos, neg, ntc = (int(v) for v in misc)
    return Shape(N, Ns, Nt, ldt, L, pos, neg, ntc, forms(lp[:L + 1], rpa[:L + 1], cpa[:L + 1], Ns, N, tail_nnz)), perm


def reached(fm):
    """(fwd LPRs, bwd LPRs, tail LPR or None) of a ``forms`` result."""
    return (frozenset(x.lpr for x in fm["fwd"]), frozenset(x.lpr for x in fm["bwd"]), fm["tail"].lpr if fm["tail"] else None)


def describe(fm):
    f, b, t = reached(fm)
    return f"fwd{{{','.join(map(str, sorted(f)))}}} bwd{{{','.join(map(str, sorted(b)))}}} tail {t if t else '-'}"


# ---------------------------------------------------------------------------------------------------------------------
# The cases.  shape: (N, Ns, Nt, ldt, levels, tail rows with sign +, with sign -); fwd / bwd / tail: the forms the case claims to reach.
# ---------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "name kind args max_tail min_level shape fwd bwd tail")

CASES = [
    Case("dense1100x30-notail", "dense", (1100, 30), 100, 1, (1130, 1130, 0, 0, 1101, 0, 0), (16, 64, 256), (1, 4, 16, 64, 256), None),
    Case("dense1100x30-tail64", "dense", (1100, 30), 64, 64, (1130, 1066, 64, 64, 1037, 64, 0), (16, 64, 256), (16, 64, 256), 256),
    Case("dense40x60", "dense", (40, 60), 100, 1, (100, 100, 0, 0, 41, 0, 0), (16, 64), (1, 4, 16), None),
    Case("dense300x30-tail64", "dense", (300, 30), 64, 64, (330, 266, 64, 64, 237, 64, 0), (16, 64), (16, 64), 64),
    Case("blocks37x12x20", "blocks", (37, 12, 20), 64, 64, (1184, 1147, 37, 64, 24, 0, 37), (4, 16), (1, 4, 16), 16),
    Case("blocks3x100x1100", "blocks", (3, 100, 1100), 250, 64, (3600, 3351, 249, 256, 18, 249, 0), (256,), (16, 64), 256),
    Case("banded600x5", "banded", (600, 5), 192, 64, (1199, 1011, 188, 192, 59, 90, 98), (1, 4), (4, 16), 16),
    Case("banded2000x8", "banded", (2000, 8), 300, 64, (3999, 3702, 297, 320, 119, 151, 146), (1, 4, 16, 64), (4, 16), 16),
]
REPEAT_CASES = ("dense40x60", "banded600x5")                          # two linsys_solve calls on the same inputs: bit-identical
PANEL_CASES = ("dense40x60", "blocks37x12x20", "banded600x5")          # through QuadraticProgramSparseSharedBatch, QPS_LDL_PANEL_SPR unset
PANEL_COUNT, PANEL_K, PANEL_PERIOD = 17, 20, 10                        # two panels, the second with one live column; fixed iterations; a check every 10
EMU_RECOMPUTED = ("dense40x60", "blocks37x12x20")                      # the two cheapest emulations, recomputed by the CPU guard


def find(name):
    return next(c for c in CASES if c.name == name)


def case_env(case):
    return {"QPS_LDL_MAX_TAIL": str(case.max_tail), "QPS_LDL_MIN_LEVEL": str(case.min_level)}


def case_limits(case):
    return (case.max_tail, case.min_level, DEFAULT_LIMITS[2])


def case_label(case):
    t = case.tail if case.tail else "-"
    return f"{case.name} fwd{{{','.join(map(str, case.fwd))}}} bwd{{{','.join(map(str, case.bwd))}}} tail {t}"


def _dense_block(rng, n1, m1):
    M, G = rng.standard_normal((n1, n1)), rng.standard_normal((m1, n1))
    return M.T @ M / n1 + np.eye(n1), G / math.sqrt(n1)


def banded_problem(n, bw, rng):
    """_banded_problem of tests/test_gpu_ldl.py (SPD band matrix, chain constraints), restated so that this module imports no test module."""
    diags = [rng.standard_normal(n - k) * 0.3 for k in range(1, bw + 1)]
    P = sp.diags([np.full(n, 2.0 * bw)] + diags + diags, [0] + list(range(1, bw + 1)) + [-k for k in range(1, bw + 1)], format="csc")
    A = sp.diags([-np.ones(n - 1), np.ones(n - 1)], [0, 1], shape=(n - 1, n), format="csc")
    return P, rng.standard_normal(n), A, -np.ones(n - 1), np.ones(n - 1)


@functools.lru_cache(maxsize=None)
def problem(name):
    """(P, q, A, l, u) of a case, P and A in CSC with sorted indices; cached, treat as read-only."""
    case = find(name)
    rng = make_rng(2024, CASES.index(case))
    if case.kind == "banded":
        P, q, A, l, u = banded_problem(*case.args, rng)
    else:
        k, n1, m1 = (1,) + case.args if case.kind == "dense" else case.args
        blocks = [_dense_block(rng, n1, m1) for _ in range(k)]
        P = sp.block_diag([sp.csc_matrix(b[0]) for b in blocks], format="csc")
        A = sp.block_diag([sp.csc_matrix(b[1]) for b in blocks], format="csc")
        q, l, u = rng.standard_normal(k * n1), -np.ones(k * m1), np.ones(k * m1)
    P, A = sp.csc_matrix(P), sp.csc_matrix(A)
    P.sort_indices(); A.sort_indices()
    return P, q, A, l, u


@functools.lru_cache(maxsize=None)
def step_inputs(name):
    """The (x, z, y) of the four steps of a case; cached, treat as read-only."""
    P, _, A, _, _ = problem(name)
    rng = make_rng(78, CASES.index(find(name)))
    return tuple((rng.standard_normal(P.shape[0]), rng.standard_normal(A.shape[0]), rho * rng.standard_normal(A.shape[0])) for _, rho in STEPS)


def panel_family(name):
    """(P, A, Q, L, U) of a panel case: PANEL_COUNT columns on the case's matrices, q ~ N(0, 1), l = s - U(0, 1), u = s + U(0, 1) around s = A x0."""
    P, _, A, _, _ = problem(name)
    n, m = P.shape[0], A.shape[0]
    rng = make_rng(79, CASES.index(find(name)))
    Q, L, U = np.zeros((PANEL_COUNT, n)), np.zeros((PANEL_COUNT, m)), np.zeros((PANEL_COUNT, m))
    for b in range(PANEL_COUNT):
        Q[b] = rng.standard_normal(n)
        s = A @ (rng.standard_normal(n) / math.sqrt(n))
        L[b], U[b] = s - rng.random(m), s + rng.random(m)
    return P, A, Q, L, U


# ---------------------------------------------------------------------------------------------------------------------
# Reference and fp32 emulation
# ---------------------------------------------------------------------------------------------------------------------
def rel(a, b):
    return np.abs(a - b).max() / max(1.0, np.abs(b).max()) if b.size else 0.0


def kkt(P, A, rho, sigma):
    n, m = P.shape[0], A.shape[0]
    return sp.bmat([[sp.csc_matrix(P) + sigma * sp.eye(n), sp.csc_matrix(A).T], [sp.csc_matrix(A), -sp.eye(m) / rho]], format="csc")


def rhs_of(q, x, z, y, rho, sigma):
    return np.concatenate([sigma * x - q, z - y / rho])               # LinearSystemSolvers.jl:37-38


def reference_solve(P, A, rho, sigma, rhs):
    """K sol = rhs in fp64 with one step of iterative refinement: dense LU where K is mostly full, sparse LU otherwise."""
    K = kkt(P, A, rho, sigma)
    N = K.shape[0]
    if K.nnz > 0.2 * N * N:
        Kd = K.toarray()
        lu = sla.lu_factor(Kd)
        solve = lambda r: sla.lu_solve(lu, r)                         # noqa: E731
    else:
        solve = spla.splu(K).solve
    sol = solve(rhs)
    return sol + solve(rhs - K @ sol)


_refs = {}


def reference(name, step):
    """(x~, z~) of one step of a case, computed once and shared; treat as read-only."""
    if (name, step) not in _refs:
        P, q, A, _, _ = problem(name)
        x, z, y = step_inputs(name)[step]
        rho = STEPS[step][1]
        sol = reference_solve(P, A, rho, SIGMA, rhs_of(q, x, z, y, rho, SIGMA))
        _refs[(name, step)] = (sol[:P.shape[0]], z + (sol[P.shape[0]:] - y) / rho)      # LinearSystemSolvers.jl:40
    return _refs[(name, step)]


def emulate_f32(Kp, rhs):
    """Kp sol = rhs by L D L' without pivoting and the two substitutions, all in numpy.float32 with sequential sums and elementwise operations only, so that
    the figures do not depend on a BLAS (right-looking: entry (i, j) takes its
    updates in the order of k, as a row-wise dot product would).  Kp: the permuted KKT matrix, dense; only the rows that a column reaches are touched, so a
    sparse factor costs what it holds."""
    a = np.array(Kp, dtype=np.float32)
    b = np.array(rhs, dtype=np.float32)
    N = a.shape[0]
    d = np.zeros(N, dtype=np.float32)
    cols = []
    for k in range(N):
        d[k] = a[k, k]
        idx = k + 1 + np.flatnonzero(a[k + 1:, k])
        lk = a[idx, k] / d[k]
        cols.append((idx, lk))
        if idx.size:
            a[np.ix_(idx, idx)] -= np.outer(lk * d[k], lk)
            a[idx, k] = lk                                             # column k of L, read row-wise by the backward substitution
    for k in range(N):                                                 # L y = b: y_r takes its terms in the order of k
        idx, lk = cols[k]
        b[idx] -= lk * b[k]
    b /= d
    for i in range(N - 1, 0, -1):                                      # L' x = y: x_k takes its terms in the order of decreasing i (elementwise: no BLAS sum)
        nz = np.flatnonzero(a[i, :i])
        b[nz] -= a[i, nz] * b[i]
    return b


def emulation_errors(name):
    """[(rel x~, rel z~) per step] of the fp32 emulation of a case against its fp64 reference, in the permutation of the case's analysis."""
    case = find(name)
    P, q, A, _, _ = problem(name)
    n = P.shape[0]
    _, perm = analyze(P, A, case_limits(case))
    iperm = np.argsort(perm)
    out = []
    for step, (_, rho) in enumerate(STEPS):
        x, z, y = step_inputs(name)[step]
        Kp = kkt(P, A, rho, SIGMA).toarray()[np.ix_(perm, perm)]
        rhs = rhs_of(q, x, z, y, rho, SIGMA)[perm]
        sol = emulate_f32(Kp, rhs)[iperm]
        zz = z.astype(np.float32) + np.float32(1.0 / rho) * (sol[n:] - y.astype(np.float32))
        rx, rz = reference(name, step)
        out.append((float(rel(sol[:n].astype(np.float64), rx)), float(rel(zz.astype(np.float64), rz))))
    return out


def bounds(name, step, dtype):
    """(bound on rel x~, bound on rel z~) of one step of a case."""
    if dtype == "f64":
        return TOL_F64, TOL_F64
    ex, ez = EMU_F32[name][step]
    return FP32_MARGIN * ex, FP32_MARGIN * ez


# Error of the fp32 emulation against the fp64 reference (``emulation_errors``): (rel x~, rel z~) per step of STEPS.
EMU_F32 = {
    "dense1100x30-notail": [(1.84e-06, 2.82e-06), (4.75e-06, 6.16e-07), (3.15e-06, 4.41e-07), (2.35e-06, 2.34e-06)],
    "dense1100x30-tail64": [(2.21e-06, 2.14e-06), (4.06e-06, 7.45e-07), (4.11e-06, 7.93e-07), (1.83e-06, 2.15e-06)],
    "dense40x60": [(3.77e-07, 4.71e-07), (5.06e-07, 4.12e-07), (4.63e-07, 5.87e-07), (4.17e-07, 4.94e-07)],
    "dense300x30-tail64": [(7.03e-07, 1.50e-06), (3.73e-06, 3.28e-07), (2.88e-06, 4.85e-07), (1.49e-06, 2.56e-06)],
    "blocks37x12x20": [(2.57e-07, 6.09e-07), (8.36e-07, 6.63e-07), (7.68e-07, 1.01e-06), (2.12e-07, 2.42e-07)],
    "blocks3x100x1100": [(1.61e-06, 2.67e-06), (1.78e-06, 2.59e-06), (1.06e-06, 2.06e-06), (2.57e-06, 1.97e-06)],
    "banded600x5": [(1.10e-07, 1.08e-06), (8.04e-07, 2.24e-07), (8.67e-07, 3.09e-07), (1.56e-07, 1.34e-06)],
    "banded2000x8": [(1.00e-07, 1.59e-06), (6.83e-07, 3.28e-07), (5.84e-07, 2.71e-07), (6.76e-08, 1.67e-06)],
}


# ---------------------------------------------------------------------------------------------------------------------
# The enumeration (printed by the CPU guard and by `python tests/ldl_band_cases.py`)
# ---------------------------------------------------------------------------------------------------------------------
def shape_row(label, limits, sh):
    def fmt(launches):
        out = []
        for lpr in LPRS:
            hit = [x for x in launches if x.lpr == lpr]
            if hit:
                out.append(f"{lpr}({len(hit)}{'r' if any(x.ragged for x in hit) else ''}{'m' if any(x.rows > 1 for x in hit) else ''})")
        return " ".join(out) if out else "-"
    t = sh.forms["tail"]
    KC, ns, last = schur_slices(sh.ldt, sh.ntc)
    spr = sorted({x.spr for x in sh.forms["fwd"] + sh.forms["bwd"]} | ({t.spr} if t else set()))
    return (f"{label:34s} {limits[0]:>5}/{limits[1]:<3} N {sh.N:5d} Ns {sh.Ns:5d} Nt {sh.Nt:4d} ({sh.ldt:4d}) levels {sh.levels:4d} | fwd {fmt(sh.forms['fwd']):32s} | bwd "
            f"{fmt(sh.forms['bwd']):38s} | tail {(str(t.lpr) + ('r' if t.ragged else '')) if t else '-':5s} +{sh.pos} -{sh.neg} | slices {ns} x {KC} (last {last}) | SPR {spr}")


LEGEND = "form(levels, r = a ragged level among them, m = a level of more than one row among them); tail: form, r = ragged; slices: K slices x KC columns"


def pair_case_rows():
    """The enumeration over PAIR_CASES of tests/test_gpu_ldl.py under the default limits: what test_ldl_plugin_pair_in_isolation reaches."""
    from quadraticprogramsolver_amd.generator import GenerateRandomQP
    from test_gpu_ldl import PAIR_CASES
    rows = []
    for pc, n in PAIR_CASES:
        P, _, A, _, _ = GenerateRandomQP(pc, n, rng=make_rng(77, int(pc)))
        sh, _ = analyze(P, A)
        rows.append((f"{pc.name} {n}", sh))
    return rows


if __name__ == "__main__":
    print(LEGEND)
    for c in CASES:
        P, _, A, _, _ = problem(c.name)
        print(shape_row(c.name, case_limits(c), analyze(P, A, case_limits(c))[0]))
    for label, sh in pair_case_rows():
        print(shape_row("PAIR " + label, DEFAULT_LIMITS, sh))
    print("EMU_F32 = {")
    for c in CASES:
        print(f'    "{c.name}": [' + ", ".join(f"({ex:.2e}, {ez:.2e})" for ex, ez in emulation_errors(c.name)) + "],")
    print("}")
