"""Cases and references of the adjoint derivatives on the shared-matrix batches (qps_adjoint_shared): what tests/test_adjoint_cpu.py guards and
tests/test_gpu_adjoint.py runs on the device.  No device is needed here.

Per column, from a solution x, multipliers y (thresholded at |y| > 1e-7, tests/shared_polish_cases.py) and g = dloss/dx: the active sets L = {y < 0}, U = {y > 0},
K = [P, A_L', A_U'; A_L, 0, 0; A_U, 0, 0], K r = [g; 0], r_lambda written back at full length m, and

    dq = -r_x,   dl = r_lambda on L,   du = r_lambda on U,   dP_ij = -(r_x,i x_j + r_x,j x_i) / 2,   dA_ij = -(y_i r_x,j + r_lambda,i x_j)

on the stored entries, dP and dA summed over the columns.  The REFERENCE solves K r = [g; 0] directly (dense solve, sparse LU for sparse matrices); the
RESTATEMENT runs the refinement rounds of the polishing step (oracle/polish_oracle_np.py: MINRES on K + delta blkdiag(I, -I)) on that right-hand side, as the
device does.  Both sides of every comparison get the same x, y and g.

The bounds of the device tests are not chosen: BOUNDS holds, per case and output, the worst distance of the restatement from the reference on this CPU, relative
to max(1, |reference|_inf); the device gets MARGIN = 4 times that, the margin of the staged polish test (both stop at the first iterate under the same relative
residual).  The figures were produced by

    python -c "import sys; sys.path[:0] = ['.', 'tests']; import adjoint_cases as c; c.print_measurements()"

Everything here is computed once per process and shared; nobody changes what these functions return."""
import functools

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import shared_polish_cases as polish_cases
from cg_shared_cases import LONG_N, banded_family
from equilibration_cases import ruiz_pow2, scrambled_sparse_family
from oracle import polish_oracle_np, qps_oracle_np
from polish_band_cases import minres_t

PARITY = polish_cases.PARITY
MARGIN = 4.0
OUTPUTS = ("dQ", "dL", "dU", "vP", "vA")
EQUIL_PASSES = polish_cases.EQUIL_PASSES
FP32 = dict(numItrPolish=10, δ=1e-6, ϵMinres=1e-3, numItrMinres=4000)          # the settings of the fp32 test (those of the fp32 polish test)

# The per-column flag test: family "dense", count 20 (on a sparse handle, which gives vP and vA), numItrPolish = 1, numItrMinres = FLAG_CAP.  First-call MINRES counts of the restatement at the parity
# tolerance (print_measurements): the columns of FLAG_COLUMNS_OVER need more than the cap, every other column fewer, all by more than 20 % of the cap.
# Counts: [921, 432, 542, 406, 344, 378, 323, 312, 342, 307, 276, 277, 296, 274, 283, 304, 270, 246, 259, 274]; 720 - 20 % = 576 >= 542, 720 + 20 % = 864 <= 921.
FLAG_CASE = ("dense", 20)
FLAG_CAP = 720
FLAG_COLUMNS_OVER = (0,)

# Worst distance of the restatement from the reference, per case and output (see the module docstring), rounded up to three digits.
BOUNDS = {
    "dense-3": {"dQ": 1.24e-15, "dL": 1.44e-14, "dU": 1.65e-14, "vP": 1.71e-16, "vA": 4.66e-15},
    "dense-20": {"dQ": 1.24e-15, "dL": 1.44e-14, "dU": 1.65e-14, "vP": 2.88e-16, "vA": 5.86e-15},
    "dense-37": {"dQ": 1.24e-15, "dL": 1.44e-14, "dU": 1.65e-14, "vP": 4.23e-16, "vA": 6.00e-15},
    "random-3": {"dQ": 2.26e-15, "dL": 1.94e-15, "dU": 2.77e-15, "vP": 2.19e-15, "vA": 2.20e-15},
    "random-20": {"dQ": 1.70e-14, "dL": 1.48e-14, "dU": 1.36e-14, "vP": 9.16e-15, "vA": 1.07e-14},
    "random_zero_y-3": {"dQ": 7.94e-14, "dL": 0.0, "dU": 0.0, "vP": 3.59e-14, "vA": 0.0},
    "banded-3": {"dQ": 3.05e-16, "dL": 2.28e-16, "dU": 3.99e-16, "vP": 3.91e-16, "vA": 2.52e-16},
    "banded71-3": {"dQ": 3.34e-16, "dL": 2.35e-16, "dU": 2.66e-16, "vP": 4.40e-16, "vA": 2.62e-16},
    "banded_long-3": {"dQ": 6.74e-16, "dL": 5.47e-16, "dU": 4.99e-16, "vP": 4.43e-16, "vA": 4.83e-16},
    "scrambled-4-equilibrated": {"dQ": 1.98e-14, "dL": 3.04e-14, "dU": 2.49e-14, "vP": 5.04e-15, "vA": 3.05e-14},
    "scrambled_random-4-equilibrated": {"dQ": 1.32e-14, "dL": 1.08e-14, "dU": 8.80e-14, "vP": 2.14e-15, "vA": 5.08e-15},
    "dense-20-flag": {"dQ": 1.40e-07, "dL": 1.74e-06, "dU": 2.09e-06, "vP": 3.88e-08, "vA": 5.71e-07},
    "dense-3-fp32": {"dQ": 1.32e-08, "dL": 1.82e-07, "dU": 2.41e-07, "vP": 1.76e-09, "vA": 6.45e-08},
    "random-3-fp32": {"dQ": 8.07e-07, "dL": 9.79e-07, "dU": 1.06e-06, "vP": 8.01e-07, "vA": 7.85e-07},
}


def gx(b, n):
    return np.random.default_rng(3 + b).standard_normal(n)


def GX(count, n):
    return np.ascontiguousarray(np.stack([gx(b, n) for b in range(count)]))


def canonical_pattern(P, A):
    """(P_indptr, P_indices, A_indptr, A_indices) of the CSC form the handles are created on: rows sorted inside every column, zeros of a dense matrix dropped."""
    out = []
    for M in (P, A):
        M = sp.csc_matrix(M).copy()
        M.sum_duplicates(); M.sort_indices()
        out += [M.indptr.astype(np.int64), M.indices.astype(np.int64)]
    return tuple(out)


def _columns_of(indptr):
    return np.repeat(np.arange(indptr.size - 1), np.diff(indptr))


def solve_direct(P, A, y, g):
    """r = (r_x [n], r_lambda [m], zero outside the active sets) of K r = [g; 0]."""
    Lo, Up = y < 0, y > 0
    act = np.concatenate([np.flatnonzero(Lo), np.flatnonzero(Up)])
    n, m = P.shape[0], A.shape[0]
    rhs = np.concatenate([g, np.zeros(act.size)])
    if sp.issparse(P):
        Aa = sp.csr_matrix(A)[act]
        K = sp.bmat([[sp.csc_matrix(P), Aa.T], [Aa, None]], format="csc") if act.size else sp.csc_matrix(P)
        s = spla.splu(K).solve(rhs)
    else:
        Aa = np.asarray(A)[act]
        s = np.linalg.solve(np.block([[P, Aa.T], [Aa, np.zeros((act.size, act.size))]]), rhs)
    rl = np.zeros(m)
    rl[act] = s[n:]
    return s[:n], rl


def outputs(rx, rl, x, y, pattern=None):
    """The six formulas for one column; vP / vA on ``pattern`` (canonical_pattern), None without one."""
    out = dict(dQ=-rx, dL=np.where(y < 0, rl, 0.0), dU=np.where(y > 0, rl, 0.0), vP=None, vA=None)
    if pattern is not None:
        Pcp, Pri, Acp, Ari = pattern
        Pj, Aj = _columns_of(Pcp), _columns_of(Acp)
        out["vP"] = -0.5 * (rx[Pri] * x[Pj] + rx[Pj] * x[Pri])
        out["vA"] = -(y[Ari] * rx[Aj] + rl[Ari] * x[Aj])
    return out


def restate(P, A, y, g, *, numItrPolish, δ, ϵMinres, numItrMinres, D=None, E=None, T=np.float64):
    """The refinement rounds SolveQuadraticProgram.m:307-320 on K r = [g; 0], as polish_oracle_np.Polish runs them on its own right-hand side: (r_x, r_lambda,
    flag, MINRES iterations per call).  D, E: the rounds run on D P D, E A D from D g and the result is D r~_x, E r~_lambda (the handle under equilibration).
    T = numpy.float32 rounds the matrices and every vector and scalar of MINRES to float32 (tests/polish_band_cases.py::minres_t)."""
    n, m = P.shape[0], A.shape[0]
    D = np.ones(n) if D is None else D
    E = np.ones(m) if E is None else E
    if sp.issparse(P):
        Ps = (sp.diags(D) @ sp.csr_matrix(P) @ sp.diags(D)).astype(T).tocsr()
        As = (sp.diags(E) @ sp.csr_matrix(A) @ sp.diags(D)).astype(T).tocsr()
    else:
        Ps, As = (P * np.outer(D, D)).astype(T), (A * np.outer(E, D)).astype(T)
    Ats = As.T.tocsr() if sp.issparse(As) else As.T
    mask = ((y < 0) | (y > 0)).astype(T)
    gv = np.concatenate([D * g, np.zeros(m)]).astype(T)

    def K(t, delta):
        tx, tl = t[:n], t[n:] * mask
        return np.concatenate([Ps @ tx + Ats @ tl + T(delta) * tx, mask * (As @ tx) - T(delta) * tl]).astype(T)

    t, tt, flag, counts = np.zeros(n + m, T), np.zeros(n + m, T), -1, []
    for _ in range(numItrPolish):
        rhs = gv - K(t, 0.0)
        if T is np.float64:
            tt, flag, _, it = polish_oracle_np.minres(lambda v: K(v, δ), rhs, ϵMinres, numItrMinres, tt)
        else:
            tt, flag, _, it = minres_t(lambda v: K(v, δ), rhs, ϵMinres, numItrMinres, tt, T)
        counts.append(it)
        if flag:
            break
        t = t + tt
    t = t.astype(np.float64)
    return D * t[:n], E * t[n:], flag, counts


# ---- the cases -------------------------------------------------------------------------------------------------------------------------------------------
# name -> (family, count, kind of handle, sparse reference); (X, Y) of the first four are ADMM states of the restatement's loop (shared_polish_cases.state), those
# of the banded families are synthetic: the families exist for their entry counts, not for a solve.
def _oracle_state(P, A, q, l, u):
    x = np.zeros(P.shape[0]); info = {}
    qps_oracle_np.SolveQuadraticProgramRefLoop(x, P, q, A, l, u, qps_oracle_np.RedCholInit, qps_oracle_np.RedChol, numIterations=4000, εAbs=1e-4, εRel=1e-4, ρ=0.1,
                                               adptΡ=False, info=info)
    return x, np.asarray(info["y"], dtype=np.float64)


@functools.lru_cache(maxsize=None)
def scrambled_random(count=4):
    """scrambled_sparse_family("random", count) with dense P and A, its thresholded ADMM states, and D, E of ten passes of the power-of-two rule."""
    P, A, Q, L, U = scrambled_sparse_family("random", count)
    P, A = polish_cases._dense(P), polish_cases._dense(A)
    S = [_oracle_state(P, A, Q[b], L[b], U[b]) for b in range(count)]
    X, Y = np.ascontiguousarray(np.stack([s[0] for s in S])), np.ascontiguousarray(polish_cases.threshold(np.stack([s[1] for s in S])))
    kd, ke = ruiz_pow2(P, A, EQUIL_PASSES)
    return (P, A, Q, L, U), X, Y, np.ldexp(1.0, np.asarray(kd, dtype=np.int64)), np.ldexp(1.0, np.asarray(ke, dtype=np.int64))


@functools.lru_cache(maxsize=None)
def banded(n, count=3):
    """banded_family(count, n) (P, A sparse) with a synthetic state: x ~ N(0, 1); y != 0 on the identity rows i = 0 mod 3 and on the difference rows j = 1 mod 3
    (signs alternating), so that the active rows have disjoint supports and K is regular and well conditioned."""
    P, A, Q, L, U = banded_family(count, n=n)
    m = A.shape[0]
    rng = np.random.default_rng(91)
    X = np.ascontiguousarray(rng.standard_normal((count, n)))
    Y = np.zeros((count, m))
    rows = np.concatenate([np.arange(0, n, 3), n + np.arange(1, n - 1, 3)])       # x_i with i = 0 mod 3; x_j+1 - x_j with j = 1 mod 3, i.e. j, j + 1 = 1, 2 mod 3
    for b in range(count):
        Y[b, rows] = np.where((np.arange(rows.size) + b) % 2 == 0, -1.0, 1.0) * (0.5 + rng.random(rows.size))
    return (P, A, Q, L, U), X, Y


@functools.lru_cache(maxsize=None)
def case(name, count):
    """((P, A, Q, L, U), X, Y): P and A dense for the families of shared_polish_cases, sparse for the banded ones."""
    if name in ("dense", "random", "scrambled"):
        return (polish_cases.family(name, count),) + polish_cases.states(name, count)
    if name == "scrambled_random":
        return scrambled_random(count)[:3]
    if name == "random_zero_y":                                    # every active set empty: P r_x = g
        data, X, Y = case("random", count)
        return data, X, np.zeros_like(Y)
    return banded({"banded": 70, "banded71": 71, "banded_long": LONG_N}[name], count)


@functools.lru_cache(maxsize=None)
def reference(name, count):
    """Per output the reference of the whole batch: dQ [count x n], dL / dU [count x m], vP / vA summed over the columns on the canonical pattern, and the
    per-column vP / vA (``vP_columns`` / ``vA_columns``) for tests that leave columns out."""
    (P, A, _, _, _), X, Y = case(name, count)
    pat = canonical_pattern(P, A)
    cols = [outputs(*solve_direct(P, A, Y[b], gx(b, P.shape[0])), X[b], Y[b], pat) for b in range(count)]
    ref = {k: np.stack([c[k] for c in cols]) for k in ("dQ", "dL", "dU")}
    ref["vP_columns"], ref["vA_columns"] = np.stack([c["vP"] for c in cols]), np.stack([c["vA"] for c in cols])
    ref["vP"], ref["vA"] = ref["vP_columns"].sum(axis=0), ref["vA_columns"].sum(axis=0)
    ref["pattern"] = pat
    return ref


def restated(name, count, settings, D=None, E=None, T=np.float64):
    """The same outputs from the restatement (flags and per-call MINRES counts per column in ``flags`` / ``counts``)."""
    (P, A, _, _, _), X, Y = case(name, count)
    pat = canonical_pattern(P, A)
    cols, flags, counts = [], [], []
    for b in range(count):
        rx, rl, flag, cnt = restate(P, A, Y[b], gx(b, P.shape[0]), D=D, E=E, T=T, **settings)
        flags.append(flag); counts.append(cnt)
        if flag:                                                   # the device gives zeros for such a column and leaves it out of the sums
            rx, rl = np.zeros_like(rx), np.zeros_like(rl)
        cols.append(outputs(rx, rl, X[b].astype(T).astype(np.float64), Y[b].astype(T).astype(np.float64), pat))
    out = {k: np.stack([c[k] for c in cols]) for k in ("dQ", "dL", "dU")}
    out["vP"], out["vA"] = np.stack([c["vP"] for c in cols]).sum(axis=0), np.stack([c["vA"] for c in cols]).sum(axis=0)
    out["flags"], out["counts"] = flags, counts
    return out


def distance(got, ref):
    """|got - ref|_inf relative to max(1, |ref|_inf); per row for a [count x len] pair, the worst row returned."""
    got, ref = np.atleast_2d(got), np.atleast_2d(ref)
    return float((np.abs(got - ref).max(axis=1) / np.maximum(1.0, np.abs(ref).max(axis=1))).max())


def bound(key, output):
    return MARGIN * BOUNDS[key][output]


def equilibration_of(name):
    """D, E of the handle after set_equilibration(EQUIL_PASSES)."""
    if name == "scrambled":
        return polish_cases.equilibrated()[1:]
    return scrambled_random()[3:]


def first_call_counts(name=None, count=None):
    """MINRES iterations of the restatement's first call at the parity tolerance, per column (default: the family of the per-column flag test)."""
    name, count = name or FLAG_CASE[0], count or FLAG_CASE[1]
    s = dict(PARITY, numItrPolish=1)
    (P, A, _, _, _), _, Y = case(name, count)
    return [restate(P, A, Y[b], gx(b, P.shape[0]), **s)[3][0] for b in range(count)]


# key -> (case name, count, settings, equilibrated, float type): what BOUNDS is measured on
MEASURED = {
    "dense-3": ("dense", 3, PARITY, False, np.float64), "dense-20": ("dense", 20, PARITY, False, np.float64), "dense-37": ("dense", 37, PARITY, False, np.float64),
    "random-3": ("random", 3, PARITY, False, np.float64), "random-20": ("random", 20, PARITY, False, np.float64),
    "random_zero_y-3": ("random_zero_y", 3, PARITY, False, np.float64),
    "banded-3": ("banded", 3, PARITY, False, np.float64), "banded71-3": ("banded71", 3, PARITY, False, np.float64),
    "banded_long-3": ("banded_long", 3, PARITY, False, np.float64),
    "scrambled-4-equilibrated": ("scrambled", 4, PARITY, True, np.float64), "scrambled_random-4-equilibrated": ("scrambled_random", 4, PARITY, True, np.float64),
    "dense-20-flag": ("dense", 20, dict(PARITY, numItrPolish=1, numItrMinres=FLAG_CAP), False, np.float64),
    "dense-3-fp32": ("dense", 3, FP32, False, np.float32), "random-3-fp32": ("random", 3, FP32, False, np.float32),
}


def measure(key):
    name, count, settings, equil, T = MEASURED[key]
    D, E = equilibration_of(name) if equil else (None, None)
    ref, res = reference(name, count), restated(name, count, settings, D, E, T)
    over = FLAG_COLUMNS_OVER if key.endswith("-flag") else ()
    assert [b for b in range(count) if res["flags"][b]] == list(over), (key, res["flags"])
    return {k: distance(res[k], flag_reference(ref, over)[k]) for k in OUTPUTS}


def flag_reference(ref, over):
    """The reference with the columns ``over`` failed: zero rows, and vP / vA summed over the other columns only."""
    keep = np.array([b not in over for b in range(ref["dQ"].shape[0])])
    out = {k: ref[k] * keep[:, None] for k in ("dQ", "dL", "dU")}
    out["vP"], out["vA"] = ref["vP_columns"][keep].sum(axis=0), ref["vA_columns"][keep].sum(axis=0)
    return out


def print_measurements():
    print("BOUNDS = {")
    for key in MEASURED:
        print(f'    "{key}": {{' + ", ".join(f'"{k}": {v:.2e}' for k, v in measure(key).items()) + "},")
    print("}")
    print("first-call MINRES counts,", FLAG_CASE, ":", first_call_counts())
