"""CPU-only checks of the shared-matrix batch boundary (qps_create_dense_shared_batch / qps_update_shared_vectors): the symbols are declared,
exported and bound, bad arguments come back before any device is needed, and a GPU-less machine gets QPS_ERR_NO_DEVICE."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("qps_create_dense_shared_batch", "qps_update_shared_vectors")
BAD_ARGUMENT, BAD_DIMENSION, NOT_FINITE, NO_DEVICE, UNSUPPORTED = 1, 2, 3, 7, 8


def _problem(count=3, n=5, m=4):
    rng = np.random.default_rng(3)
    M = rng.standard_normal((n, n))
    P = np.asfortranarray(M.T @ M + np.eye(n))
    P = np.asfortranarray(0.5 * (P + P.T))
    A = np.asfortranarray(rng.standard_normal((m, n)))
    q = np.ascontiguousarray(rng.standard_normal((count, n)))
    l = np.ascontiguousarray(-np.ones((count, m)))
    u = np.ascontiguousarray(np.ones((count, m)))
    return P, A, q, l, u


def _g(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def _create(L, count, n, m, P, ldp, A, lda, q, l, u, dtype=0, out=True):
    h = C.c_void_p()
    rc = L.qps_create_dense_shared_batch(count, n, m, _g(P), ldp, _g(A), lda, _g(q), _g(l), _g(u), dtype, 0, C.byref(h) if out else None)
    return rc, h


def test_symbols_are_declared_exported_and_bound(qps):
    from quadraticprogramsolver_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qps.h")).read(), flags=re.S)
    L = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in include/qps.h"
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(L, name), f"{name} is not exported by the library"
        fn = getattr(_lib.lib(), name)
        assert fn.restype is C.c_int32 and fn.argtypes
        assert not re.search(r"\d", name)      # the header test's pattern is qps_[a-z_]+
    assert len(_lib.lib().qps_create_dense_shared_batch.argtypes) == 13
    assert len(_lib.lib().qps_update_shared_vectors.argtypes) == 4
    assert hasattr(qps, "QuadraticProgramSharedBatch")


def test_bad_arguments_come_back_before_a_device_is_needed(qps):
    from quadraticprogramsolver_amd import _lib
    L = _lib.lib()
    P, A, q, l, u = _problem()
    count, n, m = q.shape[0], P.shape[0], A.shape[0]
    ok = (count, n, m, P, n, A, m, q, l, u)

    def with_(**kw):
        names = ("count", "n", "m", "P", "ldp", "A", "lda", "q", "l", "u")
        return tuple(kw.get(k, v) for k, v in zip(names, ok))

    # null pointers
    for name in ("P", "A", "q", "l", "u"):
        assert _create(L, *with_(**{name: None}))[0] == BAD_ARGUMENT, name
    assert _create(L, *ok, out=False)[0] == BAD_ARGUMENT
    # count <= 0
    for c in (0, -2):
        assert _create(L, *with_(count=c))[0] == BAD_DIMENSION
    assert b"count" in L.qps_last_error(None)
    # dimensions and leading dimensions
    assert _create(L, *with_(n=0))[0] == BAD_DIMENSION
    assert _create(L, *with_(ldp=n - 1))[0] == BAD_DIMENSION
    assert _create(L, *with_(lda=m - 1))[0] == BAD_DIMENSION
    assert _create(L, *ok, dtype=7)[0] == BAD_ARGUMENT
    # NaN in ONE column's q; NaN (but not Inf) in one column's bounds
    qbad = q.copy(); qbad[count - 1, 2] = np.nan
    assert _create(L, *with_(q=qbad))[0] == NOT_FINITE
    assert b"q" in L.qps_last_error(None)
    ubad = u.copy(); ubad[1, 0] = np.nan
    assert _create(L, *with_(u=ubad))[0] == NOT_FINITE
    Pnan = P.copy(order="F"); Pnan[1, 1] = np.inf
    assert _create(L, *with_(P=Pnan))[0] == NOT_FINITE
    # asymmetric P (one ulp, tolerance 0 as SolveQuadraticProgram.m:166-168)
    Pbad = P.copy(order="F"); Pbad[3, 1] = np.nextafter(Pbad[3, 1], np.inf)
    assert _create(L, *with_(P=Pbad))[0] == BAD_ARGUMENT
    assert b"symmetric" in L.qps_last_error(None)
    # what the shared path does not offer is refused by name, also before a device is needed
    rc, _ = _create(L, count, n, 0, P, n, None, 1, q, None, None)
    assert rc == UNSUPPORTED and b"m >= 1" in L.qps_last_error(None)
    # the vector update needs a shared-batch handle
    assert L.qps_update_shared_vectors(None, _g(q), None, None) == BAD_ARGUMENT


def test_python_wrapper_validates_shapes(qps):
    P, A, q, l, u = _problem()
    with pytest.raises(ValueError):
        qps.QuadraticProgramSharedBatch(P, A, q, l[:, :-1], u)
    with pytest.raises(ValueError):
        qps.QuadraticProgramSharedBatch(P, A, q[:, :-1], l, u)
    with pytest.raises(ValueError):
        qps.QuadraticProgramSharedBatch(P, A, q, l[:-1], u)


def test_good_arguments_reach_the_device_test(qps):
    """Infinite bounds are legal (l = -Inf); without a GPU the valid call fails loudly with QPS_ERR_NO_DEVICE, there is no CPU fallback."""
    from quadraticprogramsolver_amd import _lib
    L = _lib.lib()
    P, A, q, l, u = _problem()
    l[1, :] = -np.inf
    rc, h = _create(L, q.shape[0], P.shape[0], A.shape[0], P, P.shape[0], A, A.shape[0], q, l, u)
    if L.qps_device_count() == 0:
        assert rc == NO_DEVICE and not h.value
        with pytest.raises(qps.QpsError) as e:
            qps.QuadraticProgramSharedBatch(P, A, q, l, u)
        assert e.value.status == NO_DEVICE
    else:
        assert rc == 0 and h.value
        assert L.qps_destroy(h) == 0
