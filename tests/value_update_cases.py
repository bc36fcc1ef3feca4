"""Values-only update of the sparse shared-matrix batches (qps_get_shared_pattern, qps_update_shared_values): the families of tests/matrix_update_cases.py read
as value vectors in the order of the canonical pattern, the one-sided pattern, and the refused value vectors with the workgroup of the validation kernel every bad
entry is placed in.  Plain importable helper, no device needed: tests/test_value_update_cpu.py guards it, tests/test_gpu_value_update.py and
tests/tools/gpu_value_update_timing.py run the device on it."""
import numpy as np
import scipy.sparse as sp

import matrix_update_cases as mc

W = 256                                # qps_kernels.h: VALIDATE_VALUES_THREADS, entries per workgroup of the validation
KEYS = mc.SPARSE_KEYS + mc.CG_KEYS
F32_KEYS = (mc.RANDOM, mc.CG_BANDED)
CLASSES = {"sparse": "QuadraticProgramSparseSharedBatch", "cg": "QuadraticProgramCgSharedBatch"}
FIXED = dict(numIterations=mc.FIXED_ITERATIONS, ϵAbs=0.0, ϵRel=0.0, ρ=mc.RHO)        # the one-sided handles: a fixed count, nothing has to converge


def values(key, k):
    """(vP, vA) of step k in the order of the canonical pattern: what update_values takes.  Fresh copies."""
    P, A = mc.matrices(key, k)
    return mc.canonical(P).data.copy(), mc.canonical(A).data.copy()


def with_values(M, v):
    """The matrix on the canonical pattern of M with the values v: what update_matrices takes for the same update."""
    c = mc.canonical(M)
    return sp.csc_matrix((np.asarray(v, dtype=np.float64), c.indices.copy(), c.indptr.copy()), shape=c.shape)


def columns_of(c):
    return np.repeat(np.arange(c.shape[1]), np.diff(c.indptr))


def workgroup(k):
    return int(k) // W


def position(c, i, j):
    """Where entry (i, j) of the canonical matrix c is stored, or -1."""
    lo, hi = c.indptr[j], c.indptr[j + 1]
    at = lo + int(np.searchsorted(c.indices[lo:hi], i))
    return int(at) if at < hi and c.indices[at] == i else -1


_ONE_SIDED = {}


def one_sided():
    """P of mc.RANDOM with an explicit 0.0 stored at one structurally empty (i, j), i < j, and nothing stored at (j, i).  Returns (P1, k0, i, j): the matrix
    (built from (data, indices, indptr), so the zero stays stored) and the position of the zero in canonical order.  Computed once."""
    if not _ONE_SIDED:
        c = mc.canonical(mc.matrices(mc.RANDOM, 0)[0])
        n = c.shape[0]
        i, j = next((i, j) for j in range(n - 1, 0, -1) for i in range(j) if position(c, i, j) < 0 and position(c, j, i) < 0)
        k0 = c.indptr[j] + int(np.searchsorted(c.indices[c.indptr[j]:c.indptr[j + 1]], i))
        indptr = c.indptr.copy()
        indptr[j + 1:] += 1
        P1 = sp.csc_matrix((np.insert(c.data, k0, 0.0), np.insert(c.indices, k0, i), indptr), shape=c.shape)
        _ONE_SIDED["v"] = (P1, int(k0), int(i), int(j))
    return _ONE_SIDED["v"]


def _off_diagonal_in_column(c, j, which=0):
    ks = [k for k in range(c.indptr[j], c.indptr[j + 1]) if c.indices[k] != j]
    return ks[which]


def not_finite_cases():
    """(name, key, vP, vA, where): value vectors of step 1 with NaN / Inf placed; where = [(matrix, k)] names every placed entry."""
    out = []
    vP, vA = values(mc.RANDOM, 1)
    for k in (0, W - 1, W, len(vP) - 1):
        p = vP.copy()
        p[k] = np.nan
        out.append((f"random-P-nan-{k}", mc.RANDOM, p, None, [("P", k)]))
    sP, _ = values(mc.CG_SMALL, 1)
    sP[33] = np.nan
    out.append(("cg-small-P-nan-33", mc.CG_SMALL, sP, None, [("P", 33)]))
    for k in (0, len(vA) - 1):
        a = vA.copy()
        a[k] = np.inf if k == 0 else -np.inf
        out.append((f"random-A-inf-{k}", mc.RANDOM, vP.copy(), a, [("A", k)]))      # a good P beside it must not get in
    p = vP.copy()
    p[5], p[3 * W + 7] = np.nan, np.nan
    out.append(("random-P-nan-two-workgroups", mc.RANDOM, p, None, [("P", 5), ("P", 3 * W + 7)]))
    p = vP.copy()
    c = mc.canonical(mc.matrices(mc.RANDOM, 1)[0])
    p[_off_diagonal_in_column(c, 0)] *= 1.5                                          # asymmetric as well: the NaN is what gets reported
    p[20 * W + 3] = np.nan
    out.append(("random-P-nan-and-asymmetric", mc.RANDOM, p, None, [("P", 20 * W + 3)]))
    return out


def asymmetric_cases():
    """(name, vP, changed): value vectors of P of mc.RANDOM, step 1, with entries changed on one side only; changed = [k]."""
    vP, _ = values(mc.RANDOM, 1)
    c = mc.canonical(mc.matrices(mc.RANDOM, 1)[0])
    n = c.shape[0]
    out = []
    for name, j in (("first-column", 0), ("last-column", n - 1)):
        k = _off_diagonal_in_column(c, j)
        p = vP.copy()
        p[k] *= 1.5
        out.append((name, p, [k]))
    # two pairs: the changed entry of the pair with the SMALLER column lies in a later workgroup than the changed entry of the other pair
    cols = columns_of(c)
    k_hi = next(k for k in range(len(vP) - 1, -1, -1) if c.indices[k] < 10 and cols[k] > c.indices[k])          # (i < 10, j large): reported as column i
    k_lo = next(k for k in range(len(vP)) if 30 <= cols[k] < c.indices[k])                                       # (i > j >= 30) in an early workgroup
    p = vP.copy()
    p[k_hi] *= 1.25
    p[k_lo] *= 0.75
    out.append(("two-pairs", p, [k_lo, k_hi]))
    return out


def reported_column(c, v):
    """The column layout::csc_asymmetry names for the values v on the canonical pattern c (numpy restatement: the minimum, over offending entries, of
    min(i, j)), or -1."""
    D = sp.csc_matrix((np.ones(c.nnz), c.indices, c.indptr), shape=c.shape).toarray() != 0
    V = sp.csc_matrix((v, c.indices, c.indptr), shape=c.shape).toarray()
    bad = (V != V.T) & (D | D.T)
    if not bad.any():
        return -1
    i, j = np.nonzero(bad)
    return int(np.minimum(i, j).min())
