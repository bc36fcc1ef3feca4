"""Families of QPs on one sparse mP and mA for the matrix-free CG shared-matrix batch (qps_create_csc_shared_batch_cg), and a restatement of how
k_cg_panel.hip picks its strip counts and launch geometry: what tests/test_cg_shared_cpu.py, tests/test_gpu_cg_shared_batch.py and
tests/tools/gpu_cg_shared_batch_timing.py share."""
import math

import numpy as np
import scipy.sparse as sp

from quadraticprogramsolver_amd.generator import make_rng
from sparse_shared_cases import RANDOM_FAMILY_ORACLE_ITERATIONS, random_family  # noqa: F401  (re-exported)

COUNT = 20                      # two panels, 12 padding columns
RHO = {"random": 0.1, "banded": 1.0}
EPS_PCG_TIGHT, ITR_PCG_TIGHT = 1e-13, 5000


def banded_family(count, n=70):
    """P = tridiag(-1, 2.5, -1), A = [I_n; first differences] (m = 2 n - 1, at most 3 entries per row of P, 2 per row of A, 3 per row of A'); per column b,
    from make_rng(79, 1): q ~ N(0,1), x0 ~ N(0,1), s = A x0, l = s - (0.2 + 0.1 b) U(0,1), u = s + (0.2 + 0.1 b) U(0,1).  Column 1 has u = +Inf, column 2
    has l = u on its first five rows."""
    P = sp.diags([-np.ones(n - 1), 2.5 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1], format="csc")
    D = sp.diags([-np.ones(n - 1), np.ones(n - 1)], [0, 1], shape=(n - 1, n))
    A = sp.vstack([sp.eye(n), D], format="csc")
    m = A.shape[0]
    rng = make_rng(79, 1)
    Q, L, U = np.zeros((count, n)), np.zeros((count, m)), np.zeros((count, m))
    for b in range(count):
        Q[b] = rng.standard_normal(n)
        x0 = rng.standard_normal(n)
        s = A @ x0
        L[b] = s - (0.2 + 0.1 * b) * rng.random(m)
        U[b] = s + (0.2 + 0.1 * b) * rng.random(m)
        if b == 1:
            U[b] = np.inf
        if b == 2:
            L[b, :5] = U[b, :5]
    return P, A, Q, L, U


def polish_family(count):
    """banded_family with the first five rows of every column equalities (l = u = s) and every other row free.  The polishing step reads its active sets off the
    SIGN of y (SolveQuadraticProgram.m:293-299), and a row that was active and left the active set keeps a y of rounding-noise size whose sign differs between two
    correct linear-system paths; here no such row exists: a free row has y = 0 exactly in every iteration, and an equality row is the same constraint whichever
    sign its y has.  So the polished x of two handles is comparable."""
    P, A, Q, L, U = banded_family(count)
    L, U = L.copy(), U.copy()
    L[:, 5:], U[:, 5:] = -np.inf, np.inf
    U[:, :5] = L[:, :5]
    return P, A, Q, L, U


def family(name, count=COUNT):
    return random_family(count) if name == "random" else banded_family(count)


# ---- k_cg_panel.hip / panel_strips.h restated ------------------------------------------------------------------------------------------------------------
PS_THREADS, MAX_OP_BLOCKS, MAX_VEC_BLOCKS = 256, 2048, 256
LONG_N = 33000                  # banded_family(., n=LONG_N): more row groups than either launch kind has workgroups


def pick_spr(nnz, rows):
    """pick_panel_spr: strips per row from the mean row length."""
    if rows <= 0:
        return 1
    avg = nnz / rows
    return 1 if avg <= 8.0 else (4 if avg <= 64.0 else 16)


def launch_sprs(P, A):
    """The strip count of every new launch: the right-hand side walks rows of A', v = rho (A u) and the post step rows of A, the operator's second launch
    row r of P and then row r of A'."""
    n, m = P.shape[0], A.shape[0]
    pnnz, annz = sp.csc_matrix(P).nnz, sp.csc_matrix(A).nnz
    return {"rhs": pick_spr(annz, n), "av": pick_spr(annz, m), "post": pick_spr(annz, m), "op": pick_spr(pnnz + annz, n)}


def geometry(rows, spr=None):
    """(rows per workgroup and round, rounds per workgroup, workgroups per panel) of a launch that writes partials: the operator's second launch with ``spr``
    strips (at most MAX_OP_BLOCKS workgroups), or a vector kernel (``spr`` None: 16 rows per round, at most MAX_VEC_BLOCKS workgroups)."""
    rpb, cap = (16, MAX_VEC_BLOCKS) if spr is None else (PS_THREADS // (16 * spr), MAX_OP_BLOCKS)
    groups = -(-rows // rpb)
    reps = max(1, -(-groups // cap))
    return rpb, reps, -(-groups // reps)


def last_group_valid_rows(rows, spr):
    """Valid rows in the last row group of a launch (rows per group: 16 / 4 / 1)."""
    rpb = PS_THREADS // (16 * spr)
    return rows - (math.ceil(rows / rpb) - 1) * rpb
