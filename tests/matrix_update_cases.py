"""New matrices on the pattern of a shared-matrix batch (qps_update_shared_matrices, qps_update_shared_matrices_csc): the deterministic second and third matrices
of a family, the case table, and the fp32 family whose update leaves the normal range under kept exponents.  Plain importable helper, no device needed:
tests/test_matrix_update_cpu.py guards it, tests/test_gpu_matrix_update.py and tests/tools/gpu_matrix_update_timing.py run the device on it."""
import numpy as np
import scipy.sparse as sp

import cg_shared_cases as cc
import equilibration_cases as ec
import warm_start_cases as wc

REFRESH_VALUES_THREADS = 256          # qps_kernels.h: entries per workgroup of the value refresh
RHO = 0.1
PASSES = ec.PASSES
NUM_ITERATIONS = 5000
FIXED_ITERATIONS = 75                 # runs with eps = 0: three checks at numItrConv = 25

# (handle kind, family key).  "dense": QuadraticProgramSharedBatch, "sparse": QuadraticProgramSparseSharedBatch, "cg": QuadraticProgramCgSharedBatch.
CACHED, STAGED, SCRAMBLED = ("shared", 96, 160, 4), ("shared", 2112, 2304, 37), ("scrambled", 96, 160, 4)
RANDOM, LASSO, SCRAMBLED_SPARSE = ("random", 20), ("lasso", 10, 6), ("scrambled-sparse", "random", 20)
CG_RANDOM, CG_BANDED = ("cg", "random", 20), ("cg", "banded", 20)
CG_SMALL = ("cg", "banded12", 20)     # banded_family at n = 12: nnz(A) = 34, less than one wave of the value refresh
DENSE_KEYS, SPARSE_KEYS, CG_KEYS = (CACHED, STAGED, SCRAMBLED), (RANDOM, LASSO, SCRAMBLED_SPARSE), (CG_RANDOM, CG_BANDED, CG_SMALL)
UNSCALED = (CACHED, STAGED, RANDOM, LASSO, CG_RANDOM, CG_BANDED, CG_SMALL)          # the families of the fresh-handle identity
STAGED_COLS = (0, 15, 16, 31, 32, 36)


def kind_of(key):
    return "cg" if key in CG_KEYS else ("sparse" if key in SPARSE_KEYS else "dense")


def rho_of(key):
    return cc.RHO["random" if key == CG_RANDOM else "banded"] if key in CG_KEYS else RHO


def to_tolerance(key):
    """False: the tests run this family for FIXED_ITERATIONS with eps = 0 -- the staged dense family, whose restatement in numpy would take minutes; the lasso
    path, which at rho = 0.1 does not reach 1e-6 within NUM_ITERATIONS on any of its matrices (the other test modules run it at a fixed count too); the
    scrambled ones, whose exact comparison wants equal iteration counts.  True: to eps = 1e-6 within NUM_ITERATIONS."""
    return key not in (STAGED, LASSO, SCRAMBLED, SCRAMBLED_SPARSE)


def solve_kw(key):
    if to_tolerance(key):
        return dict(numIterations=NUM_ITERATIONS, ϵAbs=1e-6, ϵRel=1e-6, ρ=rho_of(key))
    return dict(numIterations=FIXED_ITERATIONS, ϵAbs=0.0, ϵRel=0.0, ρ=rho_of(key))


_DATA = {}


def data(key):
    """(P, A, Q, L, U) of a key, computed once and never changed."""
    if key not in _DATA:
        if key == CG_SMALL:
            _DATA[key] = cc.banded_family(key[2], n=12)
        elif key in CG_KEYS:
            _DATA[key] = cc.family(key[1], key[2])
        elif key[0] == "scrambled":
            _DATA[key] = ec.family(*key)
        elif key[0] == "scrambled-sparse":
            _DATA[key] = ec.family(*key[1:])
        else:
            _DATA[key] = wc.family(*key)
    return _DATA[key]


def canonical(M):
    """What the sparse classes hand to the library: scipy's CSC of M, duplicates summed (an explicit zero stays an entry)."""
    Mc = sp.csc_matrix(M, dtype=np.float64)
    Mc.sum_duplicates()
    return Mc


def step_matrices(P, A, k, pert=0.02, seed=23):
    """Deterministic matrices number k on the pattern of (P, A): A_k = A o (1 + pert R) on the stored entries, R ~ U(-1, 1); P_k = Dg P Dg with
    Dg = diag(1 + pert r) > 0, r ~ U(-1, 1), formed on the upper triangle and mirrored -- symmetric bit for bit, and a congruence, so positive semi-definite
    where P is.  Dense arrays stay dense, anything sparse comes back as canonical CSC with the index arrays of the input's canonical form."""
    rng = np.random.default_rng([seed, k])
    n = P.shape[0]
    g = 1.0 + pert * rng.uniform(-1.0, 1.0, n)
    if sp.issparse(P) or sp.issparse(A):
        Pc, Ac = canonical(P), canonical(A)
        col = np.repeat(np.arange(n), np.diff(Pc.indptr))
        lo, hi = np.minimum(Pc.indices, col), np.maximum(Pc.indices, col)          # entry (i, j) and entry (j, i) read the same upper-triangle factor
        P2 = sp.csc_matrix((Pc.data * (g[lo] * g[hi]), Pc.indices.copy(), Pc.indptr.copy()), shape=Pc.shape)
        A2 = sp.csc_matrix((Ac.data * (1.0 + pert * rng.uniform(-1.0, 1.0, Ac.nnz)), Ac.indices.copy(), Ac.indptr.copy()), shape=Ac.shape)
        return P2, A2
    P, A = np.asarray(P, dtype=np.float64), np.asarray(A, dtype=np.float64)
    T = np.triu(P * np.outer(g, g))
    return T + np.triu(T, 1).T, A * (1.0 + pert * rng.uniform(-1.0, 1.0, A.shape))


_STEPS = {}


def matrices(key, k):
    """(P_k, A_k) of a key: k = 0 the family's own, k = 1, 2 the second and third matrices.  Computed once, never changed."""
    if (key, k) not in _STEPS:
        P, A = data(key)[:2]
        _STEPS[(key, k)] = (P, A) if k == 0 else step_matrices(P, A, k)
    return _STEPS[(key, k)]


def updated_cases():
    """(key, kP, kA) of every pair of matrices a test solves to a tolerance after an update: the full update of every such family, the partial ones of one
    family per handle kind."""
    full = [(key, 1, 1) for key in UNSCALED if to_tolerance(key)]
    return full + [(key, kP, kA) for key in (CACHED, RANDOM, CG_BANDED) for kP, kA in ((1, 0), (0, 1))]


def range_case():
    """An fp32 family as equilibration_cases.out_of_range_family builds its own -- 1e4 beside A[0, 0] in its row and its column, P = 1e4 I -- in two steps:
    with A[0, 0] = 1 the scaling of PASSES passes is in range; the update to A[0, 0] = 2e-38 (a normal fp32 number) under the kept exponents is not.
    Returns (P, A1, A2, Q, L, U)."""
    P, A2, Q, L, U = ec.out_of_range_family()
    A1 = A2.copy()
    A1[0, 0] = 1.0
    return P, A1, A2, Q, L, U
