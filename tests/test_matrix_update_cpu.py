"""CPU guards of the in-place matrix update of the shared-matrix batches (qps_update_shared_matrices, qps_update_shared_matrices_csc): the two symbols through
every layer of the boundary, the cases of tests/matrix_update_cases.py -- same pattern, exact symmetry, definiteness, iteration counts of the numpy restatement,
range of the scaled entries under kept exponents, sizes around the refresh kernel's workgroup -- and the position map of the by-rows copy of A against a
brute-force search, in a stand-alone program built with AddressSanitizer and UBSan.  No device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import equilibration_cases as ec
import matrix_update_cases as mc
import warm_start_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("qps_update_shared_matrices", "qps_update_shared_matrices_csc")
BAD_ARGUMENT = 1
F32_TINY, F32_MAX = float(np.finfo(np.float32).tiny), float(np.finfo(np.float32).max)
F64_TINY, F64_MAX = float(np.finfo(np.float64).tiny), float(np.finfo(np.float64).max)
SPARSE_LIKE = mc.SPARSE_KEYS + mc.CG_KEYS
ALL_KEYS = mc.DENSE_KEYS + SPARSE_LIKE


def test_both_symbols_are_declared_exported_bound_and_called_from_julia(qps):
    from quadraticprogramsolver_amd import _lib
    header = open(os.path.join(ROOT, "include", "qps.h")).read()
    julia = re.sub(r"#[^\n]*", "", open(os.path.join(ROOT, "julia", "QuadraticProgramSolverHIP.jl"), encoding="utf-8").read())
    L = _lib.lib()
    for s in SYMBOLS:
        assert re.search(r"\bint32_t\s+%s\s*\(" % s, header), s
        assert s in _lib.EXPORTED_SYMBOLS, s
        assert getattr(L, s).argtypes is not None and getattr(L, s).restype is C.c_int32, s
        assert re.search(r"ccall\(\(:%s,\s*LIBQPS\)" % s, julia), s
    assert len(L.qps_update_shared_matrices.argtypes) == 5 and len(L.qps_update_shared_matrices_csc.argtypes) == 8


def test_a_null_handle_is_a_bad_argument(qps):
    from quadraticprogramsolver_amd import _lib
    L = _lib.lib()
    assert L.qps_update_shared_matrices(None, None, 0, None, 0) == BAD_ARGUMENT
    assert b"handle is NULL" in L.qps_last_error(None)
    assert L.qps_update_shared_matrices_csc(None, None, None, None, None, None, None, 0) == BAD_ARGUMENT
    assert b"handle is NULL" in L.qps_last_error(None)


def test_the_python_classes_have_the_method(qps):
    for cls in (qps.QuadraticProgramSharedBatch, qps.QuadraticProgramSparseSharedBatch, qps.QuadraticProgramCgSharedBatch):
        assert callable(getattr(cls, "update_matrices"))
    assert qps.QuadraticProgramSparseSharedBatch.update_matrices is not qps.QuadraticProgramSharedBatch.update_matrices


def _min_eig(P):
    return float(np.linalg.eigvalsh(ec._dense(P)).min())


@pytest.mark.parametrize("key", [k for k in ALL_KEYS if k != mc.STAGED], ids=str)
def test_step_matrices_keep_the_pattern_the_symmetry_and_the_definiteness(key):
    P0, A0 = mc.matrices(key, 0)
    for k in (1, 2):
        P, A = mc.matrices(key, k)
        assert sp.issparse(P) == (mc.kind_of(key) != "dense") and P.shape == P0.shape and A.shape == A0.shape
        if sp.issparse(P):
            for M, M0 in ((P, P0), (A, A0)):
                c, c0 = mc.canonical(M), mc.canonical(M0)
                assert np.array_equal(c.indptr, c0.indptr) and np.array_equal(c.indices, c0.indices)
                assert np.array_equal(c.data != 0, c0.data != 0)          # a stored entry keeps being one; nothing new is stored
        else:
            assert np.array_equal(A != 0, A0 != 0) and np.array_equal(P != 0, P0 != 0)
        Pd = ec._dense(P)
        assert np.array_equal(Pd, Pd.T)                                  # issymmetric with tolerance 0
        assert not np.array_equal(Pd, ec._dense(P0)) and not np.array_equal(ec._dense(A), ec._dense(A0))
        e0, e = _min_eig(P0), _min_eig(P)
        print(f"{key} step {k}: smallest eigenvalue {e0:.3e} -> {e:.3e}")
        if e0 > 0:
            assert e > 0
        else:
            assert e > -1e-12 * max(1.0, float(np.abs(Pd).max()))         # semi-definite stays semi-definite up to rounding of the congruence


def test_step_matrices_of_the_staged_family_keep_symmetry_and_pattern():
    P0, A0 = mc.matrices(mc.STAGED, 0)
    P, A = mc.matrices(mc.STAGED, 1)
    assert np.array_equal(P, P.T) and np.array_equal(A != 0, A0 != 0) and not np.array_equal(P, P0)
    # Dg P Dg is a congruence: the Cholesky factorisation that proves P0 definite proves P too
    np.linalg.cholesky(P0 + 1e-6 * np.eye(P0.shape[0]))
    np.linalg.cholesky(P + 1e-6 * np.eye(P.shape[0]))


def test_step_matrices_are_deterministic_and_differ_by_step():
    P, A = mc.data(mc.RANDOM)[:2]
    a, b, c = mc.step_matrices(P, A, 1), mc.step_matrices(P, A, 1), mc.step_matrices(P, A, 2)
    assert np.array_equal(a[0].data, b[0].data) and np.array_equal(a[1].data, b[1].data)
    assert not np.array_equal(a[0].data, c[0].data) and not np.array_equal(a[1].data, c[1].data)


@pytest.mark.parametrize("case", mc.updated_cases(), ids=str)
def test_the_restatement_stops_clear_of_num_iterations_on_every_updated_case(case):
    """Figures of the numpy restatement (reduced form for the dense handle, dense KKT form for the sparse and the CG handle), not of a device."""
    key, kP, kA = case
    _, _, Q, L, U = mc.data(key)
    P, A = mc.matrices(key, kP)[0], mc.matrices(key, kA)[1]
    R = wc.WarmRestatement(P, A, form="reduced" if mc.kind_of(key) == "dense" else "kkt")
    run = R.solve_from(Q, L, U, rho=mc.rho_of(key), numIterations=mc.NUM_ITERATIONS)
    its = [c["iterations"] for c in run["columns"]]
    print(f"{case}: iterations {its}, flags {[c['convFlag'] for c in run['columns']]}")
    assert max(its) <= 0.8 * mc.NUM_ITERATIONS
    assert all(c["convFlag"] in (2, 3) for c in run["columns"])


@pytest.mark.parametrize("key", [mc.SCRAMBLED, mc.SCRAMBLED_SPARSE], ids=str)
def test_updated_scrambled_cases_stay_normal_in_fp64_under_the_kept_exponents(key):
    P0, A0 = mc.matrices(key, 0)
    kd, ke = ec.ruiz_pow2(P0, A0, mc.PASSES)
    assert kd.any() and ke.any()                                          # a scaling that does something
    D, E = np.ldexp(1.0, kd), np.ldexp(1.0, ke)
    for k in (1, 2):
        P, A = (ec._dense(M) for M in mc.matrices(key, k))
        for S in (np.abs(D[:, None] * P * D[None, :]), np.abs(E[:, None] * A * D[None, :])):
            nz = S[S != 0]
            print(f"{key} step {k}: scaled magnitudes {nz.min():.3e} .. {nz.max():.3e}")
            assert nz.min() >= F64_TINY and nz.max() <= F64_MAX


def test_the_fp32_range_case_is_in_range_before_and_out_of_range_after_the_update():
    P, A1, A2, Q, L, U = mc.range_case()
    assert np.array_equal(A1 != 0, A2 != 0) and np.array_equal(P, P.T)
    kd, ke = ec.ruiz_pow2(P, A1, mc.PASSES, "f32")
    D, E = np.ldexp(1.0, kd), np.ldexp(1.0, ke)
    scaled = lambda A: np.abs((E[:, None] * A.astype(np.float32).astype(np.float64) * D[None, :]))
    for S in (scaled(A1), np.abs(D[:, None] * P * D[None, :])):
        assert S[S != 0].min() >= F32_TINY and S.max() <= F32_MAX          # the scaling itself is accepted
    assert F32_TINY <= abs(np.float32(A2[0, 0])) and 0 < scaled(A2)[0, 0] < F32_TINY   # a normal fp32 entry that the kept exponents push below the normal range
    S2 = scaled(A2)
    assert S2[S2 != 0].min() >= F64_TINY                                   # an fp64 handle takes the same update


def test_sparse_cases_cover_the_sizes_around_the_refresh_workgroup():
    nnzA = {key: mc.canonical(mc.matrices(key, 0)[1]).nnz for key in SPARSE_LIKE}
    nnzP = {key: mc.canonical(mc.matrices(key, 0)[0]).nnz for key in SPARSE_LIKE}
    print("nnz(A):", nnzA, "nnz(P):", nnzP)
    assert any(v % mc.REFRESH_VALUES_THREADS != 0 for v in nnzA.values())
    assert any(0 < v < 64 for v in nnzA.values())
    assert any(v > mc.REFRESH_VALUES_THREADS for v in nnzA.values())       # more than one workgroup
    header = open(os.path.join(ROOT, "quadraticprogramsolver_amd", "csrc", "qps_kernels.h")).read()
    assert re.search(r"REFRESH_VALUES_THREADS\s*=\s*%d\b" % mc.REFRESH_VALUES_THREADS, header)


def test_position_map_against_brute_force_under_asan_and_ubsan(tmp_path):
    """csc_rows_position_map of spmv_layout.cpp on the pattern of A -- and of P, read as an n x n matrix -- of every sparse case, in a stand-alone program."""
    exe, patterns = tmp_path / "position_map_check", tmp_path / "patterns.txt"
    src = [os.path.join(ROOT, "tests", "capi", "position_map_check.cpp"), os.path.join(ROOT, "quadraticprogramsolver_amd", "csrc", "spmv_layout.cpp")]
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-static-libasan", "-static-libubsan",          # the runtimes in the program itself: nothing about it depends on the load order
                            "-Wall", "-Wextra", "-o", str(exe)] + src, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    count = 0
    with open(patterns, "w") as f:
        for key in SPARSE_LIKE:
            for M in mc.matrices(key, 0):
                c = mc.canonical(M)
                f.write(f"{c.shape[0]} {c.shape[1]} {c.nnz}\n{' '.join(map(str, c.indptr))}\n{' '.join(map(str, c.indices))}\n")
                count += 1
        f.write("3 2 0\n0 0 0\n\n")                                         # an empty matrix
        f.write("1 4 4\n0 1 2 3 4\n0 0 0 0\n")                              # one row
        count += 2
    res = subprocess.run([str(exe), str(patterns)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(res.stdout)
    assert res.returncode == 0, res.stdout
    assert f"{count} patterns" in res.stdout
