"""CPU guards of the values-only update of the sparse shared-matrix batches (qps_get_shared_pattern, qps_update_shared_values): the two symbols through every
layer of the boundary, the yardsticks of tests/value_update_cases.py -- every bad entry in the workgroup of the validation kernel its case claims, the one-sided
pattern, the two asymmetric pairs -- and the transpose-partner map against a brute-force search and against layout::csc_asymmetry, in a stand-alone program built
with AddressSanitizer and UBSan.  No device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import matrix_update_cases as mc
import value_update_cases as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("qps_get_shared_pattern", "qps_update_shared_values")
BAD_ARGUMENT = 1


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
    assert len(L.qps_get_shared_pattern.argtypes) == 7 and len(L.qps_update_shared_values.argtypes) == 6
    assert re.search(r"#define\s+QPS_MEM_HOST\s+0\b", header) and re.search(r"#define\s+QPS_MEM_DEVICE\s+1\b", header)
    assert (_lib.QPS_MEM_HOST, _lib.QPS_MEM_DEVICE) == (0, 1)


def test_a_null_handle_is_a_bad_argument(qps):
    from quadraticprogramsolver_amd import _lib
    L = _lib.lib()
    assert L.qps_get_shared_pattern(None, None, None, None, None, None, None) == BAD_ARGUMENT
    assert b"handle is NULL" in L.qps_last_error(None)
    assert L.qps_update_shared_values(None, None, 0, None, 0, 0) == BAD_ARGUMENT
    assert b"handle is NULL" in L.qps_last_error(None)


def test_the_python_classes_have_both_methods(qps):
    for cls in (qps.QuadraticProgramSparseSharedBatch, qps.QuadraticProgramCgSharedBatch):
        assert callable(getattr(cls, "pattern")) and callable(getattr(cls, "update_values"))
    assert qps.QuadraticProgramCgSharedBatch.update_values is qps.QuadraticProgramSparseSharedBatch.update_values          # inherited
    assert not hasattr(qps.QuadraticProgramSharedBatch, "update_values")                                                   # the dense handle is out of scope


def test_the_workgroup_size_is_the_one_of_the_kernel_header():
    header = open(os.path.join(ROOT, "quadraticprogramsolver_amd", "csrc", "qps_kernels.h")).read()
    assert re.search(r"VALIDATE_VALUES_THREADS\s*=\s*%d\b" % vc.W, header)


def test_the_families_have_the_sizes_the_cases_are_built_for():
    nnz = {key: tuple(mc.canonical(M).nnz for M in mc.matrices(key, 0)) for key in vc.KEYS}
    print(nnz)
    assert nnz[mc.RANDOM] == (8804, 803) and nnz[mc.CG_BANDED] == (208, 208) and nnz[mc.CG_SMALL] == (34, 34) and nnz[mc.LASSO] == (1000, 2527)
    assert nnz[mc.RANDOM][0] > 34 * vc.W and nnz[mc.RANDOM][0] % vc.W != 0             # 35 workgroups, the last one partial
    assert nnz[mc.CG_BANDED][0] < vc.W and nnz[mc.CG_SMALL][0] < 64                     # less than a workgroup, less than a wave
    P = mc.canonical(mc.matrices(mc.LASSO, 0)[0])
    assert np.array_equal(P.indices, np.repeat(np.arange(P.shape[0]), np.diff(P.indptr)))          # diagonal: the partner map is the identity


def test_every_placed_bad_entry_lies_in_the_workgroup_its_case_claims():
    claims = {"random-P-nan-0": [0], f"random-P-nan-{vc.W - 1}": [0], f"random-P-nan-{vc.W}": [1], "random-P-nan-8803": [34], "cg-small-P-nan-33": [0],
              "random-A-inf-0": [0], "random-A-inf-802": [3], "random-P-nan-two-workgroups": [0, 3], "random-P-nan-and-asymmetric": [20]}
    cases = vc.not_finite_cases()
    assert sorted(c[0] for c in cases) == sorted(claims)
    for name, key, vP, vA, where in cases:
        ref = dict(zip("PA", vc.values(key, 1)))
        got = dict(P=vP, A=vA)
        assert [vc.workgroup(k) for _, k in where] == claims[name], name
        for M in "PA":
            placed = sorted(k for m, k in where if m == M)
            if got[M] is None:
                assert not placed
                continue
            assert len(got[M]) == len(ref[M])
            assert sorted(np.nonzero(~np.isfinite(got[M]))[0].tolist()) == placed, name          # exactly the placed entries are not finite
        last = {"P": len(ref["P"]) - 1, "A": len(ref["A"]) - 1}
        assert all(0 <= k <= last[m] for m, k in where)
    both = next(c for c in cases if c[0] == "random-P-nan-and-asymmetric")
    c = mc.canonical(mc.matrices(mc.RANDOM, 1)[0])
    assert vc.reported_column(c, np.nan_to_num(both[2], nan=1.0)) >= 0                            # asymmetric even without the NaN


def test_the_one_sided_pattern_is_one_sided_after_canonical():
    P1, k0, i, j = vc.one_sided()
    c, c0 = mc.canonical(P1), mc.canonical(mc.matrices(mc.RANDOM, 0)[0])
    assert i < j and c.nnz == c0.nnz + 1
    assert vc.position(c, i, j) == k0 and c.data[k0] == 0.0 and vc.position(c, j, i) == -1          # the zero is stored, its transpose is not
    assert vc.position(c0, i, j) == -1 and vc.position(c0, j, i) == -1
    assert np.array_equal(np.delete(c.data, k0), c0.data) and np.array_equal(np.delete(c.indices, k0), c0.indices)
    Pd = P1.toarray()
    assert np.array_equal(Pd, Pd.T)                                                                  # symmetric as values: creation accepts it
    v = c.data.copy()
    v[k0] = 0.25
    assert vc.reported_column(c, v) == i                                                             # column j holds the entry, column i is named


def test_the_asymmetric_cases_are_what_they_claim():
    c = mc.canonical(mc.matrices(mc.RANDOM, 1)[0])
    cols = vc.columns_of(c)
    n = c.shape[0]
    cases = {name: (vP, changed) for name, vP, changed in vc.asymmetric_cases()}
    vP0 = vc.values(mc.RANDOM, 1)[0]
    assert vc.reported_column(c, vP0) == -1
    for name, (vP, changed) in cases.items():
        assert sorted(np.nonzero(vP != vP0)[0].tolist()) == sorted(changed), name
        assert all(c.indices[k] != cols[k] for k in changed), name                                  # off-diagonal entries
    (k,) = cases["first-column"][1]
    assert cols[k] == 0 and vc.reported_column(c, cases["first-column"][0]) == 0
    (k,) = cases["last-column"][1]
    assert cols[k] == n - 1 and vc.reported_column(c, cases["last-column"][0]) == c.indices[k]
    vP, (k_lo, k_hi) = cases["two-pairs"]
    col_lo, col_hi = (min(int(c.indices[k]), int(cols[k])) for k in (k_lo, k_hi))
    assert vc.workgroup(k_lo) != vc.workgroup(k_hi) and col_lo != col_hi
    assert vc.workgroup(k_hi) > vc.workgroup(k_lo) and col_hi < col_lo                              # the smaller column sits in the later workgroup
    assert vc.reported_column(c, vP) == col_hi


def test_partner_map_against_brute_force_under_asan_and_ubsan(tmp_path):
    """csc_transpose_partner_map of spmv_layout.cpp on the pattern of P of every sparse case and of the one-sided pattern, in a stand-alone program."""
    exe, patterns = tmp_path / "partner_map_check", tmp_path / "patterns.txt"
    src = [os.path.join(ROOT, "tests", "capi", "partner_map_check.cpp"), os.path.join(ROOT, "quadraticprogramsolver_amd", "csrc", "spmv_layout.cpp")]
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-static-libasan", "-static-libubsan",          # the runtimes in the program itself: nothing about it depends on the load order
                            "-Wall", "-Wextra", "-o", str(exe)] + src, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    count = 0
    with open(patterns, "w") as f:
        for M in [mc.matrices(key, 0)[0] for key in vc.KEYS] + [vc.one_sided()[0]]:
            c = mc.canonical(M)
            f.write(f"{c.shape[0]} {c.nnz}\n{' '.join(map(str, c.indptr))}\n{' '.join(map(str, c.indices))}\n")
            count += 1
        f.write("3 0\n0 0 0 0\n\n")                                         # an empty matrix
        f.write("4 4\n0 1 2 3 4\n0 1 2 3\n")                                # a diagonal one
        f.write("4 5\n0 2 2 4 5\n0 2 0 2 3\n")                              # an empty column (and row) 1
        f.write("3 3\n0 0 2 3\n0 2 1\n")                                    # an empty first column: (0, 1) has no partner, (2, 1) and (1, 2) are a pair
        count += 4
    res = subprocess.run([str(exe), str(patterns)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(res.stdout)
    assert res.returncode == 0, res.stdout
    assert f"{count} patterns" in res.stdout
