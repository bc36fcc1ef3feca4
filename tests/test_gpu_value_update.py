"""Values-only update of the sparse shared-matrix batches on the device (qps_get_shared_pattern, qps_update_shared_values): sparse KKT L D L' and matrix-free CG
handle.  The reference is the library itself: a twin handle that takes the same values through ``update_matrices`` has to end bit for bit where the handle that
took them through ``update_values`` ends, and a refusal has to carry the status and the text of ``update_matrices`` for the same values and leave the handle
what it was.  The checks live in tests/value_update_checks.py and run twice: here from numpy arrays (QPS_MEM_HOST), and from torch device tensors
(QPS_MEM_DEVICE) in ONE child process that imports torch before the library (tests/value_update_device_child.py; one HIP runtime per process).  Families,
values and the placement of every bad entry: tests/value_update_cases.py, guarded by tests/test_value_update_cpu.py."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import matrix_update_cases as mc
import value_update_cases as vc
import value_update_checks as ck
from test_gpu_warm_start import run, same

pytestmark = pytest.mark.gpu

BAD_ARGUMENT, NOT_FINITE, UNSUPPORTED = ck.BAD_ARGUMENT, ck.NOT_FINITE, ck.UNSUPPORTED
HERE = os.path.dirname(os.path.abspath(__file__))
DEVICE_CHECKS = list(ck.CHECKS) + ["value-errors"]


# ---------------------------------------------------------------------------------------------------------------------
# 1. the pattern
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", vc.KEYS, ids=str)
def test_pattern_is_the_canonical_pattern_of_creation(gpu, key):
    P, A = mc.matrices(key, 0)
    with ck.make(gpu, key) as h:
        got = h.pattern()
    assert all(a.dtype == np.int64 for a in got)
    for (cp, ri), M in ((got[:2], P), (got[2:], A)):
        c = mc.canonical(M)
        assert np.array_equal(cp, c.indptr) and np.array_equal(ri, c.indices)


def test_pattern_of_an_unsorted_coo_matrix_with_duplicates_is_sorted_and_summed(gpu):
    key = mc.CG_BANDED
    P, A, Q, L, U = mc.data(key)
    coo = sp.coo_matrix(A)
    order = np.random.default_rng(3).permutation(coo.nnz)
    row, col, val = coo.row[order], coo.col[order], coo.data[order]
    # every entry in two halves, rows unsorted inside the columns: a CSC matrix built from raw arrays keeps both
    by_col = np.argsort(np.concatenate([col, col]), kind="stable")
    rows2, vals2 = np.concatenate([row, row])[by_col], np.concatenate([0.25 * val, 0.75 * val])[by_col]
    indptr = np.concatenate([[0], np.cumsum(np.bincount(col, minlength=A.shape[1]) * 2)])
    raw = sp.csc_matrix((vals2, rows2, indptr), shape=A.shape)
    assert not raw.has_sorted_indices and raw.nnz == 2 * coo.nnz
    c = mc.canonical(A)
    with gpu.QuadraticProgramCgSharedBatch(P, raw, Q, L, U) as h:
        Pcp, Pri, Acp, Ari = h.pattern()
        assert np.array_equal(Acp, c.indptr) and np.array_equal(Ari, c.indices)
        h.update_values(vA=vc.values(key, 1)[1])                           # values in that order, nothing about the caller's own storage
        assert np.array_equal(h.pattern()[3], c.indices)
        got = run(h, **mc.solve_kw(key))
    with gpu.QuadraticProgramCgSharedBatch(P, mc.matrices(key, 1)[1], Q, L, U) as f:
        assert same(got, run(f, **mc.solve_kw(key)))


# ---------------------------------------------------------------------------------------------------------------------
# 2. - 5. from numpy arrays
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ck.CHECKS), ids=str)
def test_from_numpy(gpu, name):
    fn, args = ck.CHECKS[name]
    fn(gpu, lambda v: v, *args)


# ---------------------------------------------------------------------------------------------------------------------
# ... and from torch device tensors
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def device_report(gpu):
    res = subprocess.run([sys.executable, os.path.join(HERE, "value_update_device_child.py")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    report = {}
    for line in res.stdout.splitlines():
        if line.startswith("{"):
            r = json.loads(line)
            report[r["check"]] = r
    return res, report


@pytest.mark.parametrize("name", DEVICE_CHECKS, ids=str)
def test_from_torch_device_tensors(device_report, name):
    res, report = device_report
    assert name in report, f"the child process reported nothing for {name} (exit code {res.returncode})\n{res.stderr[-3000:]}"
    print(report[name]["detail"])
    assert report[name]["ok"], report[name]["detail"]


# ---------------------------------------------------------------------------------------------------------------------
# 5. refusals of the arguments, 6. both NULL
# ---------------------------------------------------------------------------------------------------------------------
def _raw_values(h, vP=None, nP=0, vA=None, nA=0, location=0):
    from quadraticprogramsolver_amd import _lib
    L = _lib.lib()
    ptr = lambda a: None if a is None else a.ctypes.data
    rc = L.qps_update_shared_values(h._h, ptr(vP), nP, ptr(vA), nA, location)
    return rc, L.qps_last_error(h._h).decode()


def _raw_pattern(h):
    from quadraticprogramsolver_amd import _lib
    L = _lib.lib()
    nP, nA = C.c_int64(-7), C.c_int64(-7)
    rc = L.qps_get_shared_pattern(h._h, C.byref(nP), C.byref(nA), None, None, None, None)
    return rc, L.qps_last_error(h._h).decode(), nP.value, nA.value


@pytest.mark.parametrize("key", [mc.RANDOM, mc.CG_BANDED], ids=str)
def test_refused_arguments_leave_the_handle_untouched(gpu, key):
    vP, vA = vc.values(key, 1)
    with ck.make(gpu, key) as h:
        guard = ck.Untouched(gpu, h, mc.solve_kw(key), ck.twin_solve(gpu, key))

        def refused(what, rc_msg, code, *texts):
            rc, msg = rc_msg
            print(f"{key} {what}: {rc} {msg}")
            assert rc == code and all(t in msg for t in texts), (what, rc, msg)
            guard.check(what)

        refused("wrong nnzP", _raw_values(h, vP, len(vP) - 1, vA, len(vA)), BAD_ARGUMENT, "nnzP", str(len(vP) - 1), str(len(vP)))
        refused("wrong nnzA", _raw_values(h, vP, len(vP), vA, len(vA) + 1), BAD_ARGUMENT, "nnzA", str(len(vA) + 1), str(len(vA)))
        refused("location 2", _raw_values(h, vP, len(vP), vA, len(vA), 2), BAD_ARGUMENT, "location")
        # host memory announced as device memory: refused from the pointer attributes, on the host, before anything is enqueued
        refused("host pointer as device memory", _raw_values(h, vP, len(vP), None, 0, 1), BAD_ARGUMENT, "P_nzval is not device memory")
        refused("host pointer as device memory", _raw_values(h, None, 0, vA, len(vA), 1), BAD_ARGUMENT, "A_nzval is not device memory")
        rc, msg = _raw_values(h, None, 123, None, -1, 0)                   # both NULL: QPS_OK, the counts are ignored, the factor stays valid
        assert rc == 0, (rc, msg)
        h.update_values()
        guard.check("both NULL")
        rc, msg = _raw_values(h, vP, len(vP), vA, len(vA))                 # ... and the same arrays with the right arguments are taken
        assert rc == 0, (rc, msg)
        assert not np.array_equal(run(h, **mc.solve_kw(key))["X"], guard.before["X"])


def test_other_handles_are_refused_by_both_functions(gpu):
    from quadraticprogramsolver_amd import _lib
    Lb = _lib.lib()
    P, A, Q, L, U = mc.data(mc.CACHED)
    v = np.ones(4)
    kw = mc.solve_kw(mc.CACHED)
    with gpu.QuadraticProgramSharedBatch(P, A, Q, L, U) as h:             # the dense shared handle: its own entry point is named
        before = run(h, **kw)
        rc, msg = _raw_values(h, v, 4, None, 0)
        assert rc == UNSUPPORTED and msg == "qps_update_shared_values: a dense shared-matrix batch takes its matrices through qps_update_shared_matrices", (rc, msg)
        rc, msg, nP, nA = _raw_pattern(h)
        assert rc == UNSUPPORTED and msg.startswith("qps_get_shared_pattern: a dense shared-matrix batch") and (nP, nA) == (-7, -7), (rc, msg)
        with pytest.raises(AttributeError):
            h.update_values(v)                                             # the dense class has no such method
        assert same(run(h, reuseFactor=True, **kw), before)
    with gpu.QuadraticProgram(P, Q[0], A, L[0], U[0]) as h:               # a stand-alone handle, dense and CSC
        for fn in (lambda: _raw_values(h, v, 4, None, 0), lambda: _raw_pattern(h)[:2]):
            rc, msg = fn()
            assert rc == UNSUPPORTED and "only shared-matrix batch handles" in msg, (rc, msg)
    with gpu.QuadraticProgram(sp.csc_matrix(P), Q[0], sp.csc_matrix(A), L[0], U[0], linsys="cg") as h:
        for fn in (lambda: _raw_values(h, v, 4, None, 0), lambda: _raw_pattern(h)[:2]):
            rc, msg = fn()
            assert rc == UNSUPPORTED and "only shared-matrix batch handles" in msg, (rc, msg)
    with gpu.QuadraticProgramBatch([(P, Q[b], A, L[b], U[b]) for b in range(3)]) as h:          # a replicated batch handle (qps_create_dense_batch)
        for fn in (lambda: _raw_values(h, v, 4, None, 0), lambda: _raw_pattern(h)[:2]):
            rc, msg = fn()
            assert rc == UNSUPPORTED and "only shared-matrix batch handles" in msg, (rc, msg)
