"""CPU-only guards of the adjoint derivatives on the shared-matrix batches (qps_adjoint_shared): the bindings, the refusals that need no device, and the
reference, the cases and the MINRES cap of tests/adjoint_cases.py that tests/test_gpu_adjoint.py compares the device with."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import adjoint_cases as cases
import shared_polish_cases as polish_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARGUMENT = 1
FD_FAMILIES = (("dense", 3), ("random", 3))


def test_symbol_argtypes_and_julia_signature(qps):
    from quadraticprogramsolver_amd import _lib
    L = _lib.lib()
    assert "qps_adjoint_shared" in _lib.EXPORTED_SYMBOLS
    dp = C.POINTER(C.c_double)
    assert list(L.qps_adjoint_shared.argtypes) == [C.c_void_p, dp, dp, dp, C.POINTER(_lib.QpsParams), dp, dp, dp, dp, dp, C.POINTER(_lib.QpsPolishReport)]
    assert L.qps_adjoint_shared.restype is C.c_int32
    header = open(os.path.join(ROOT, "include", "qps.h")).read()
    assert re.search(r"\bint32_t\s+qps_adjoint_shared\s*\(\s*qps_handle\s+\w+\s*,\s*const\s+double\s*\*\s*x\s*,\s*const\s+double\s*\*\s*y\s*,\s*const\s+double\s*\*\s*gx\s*,"
                     r"\s*const\s+qps_params\s*\*\s*\w+\s*,\s*double\s*\*\s*dq\s*,\s*double\s*\*\s*dl\s*,\s*double\s*\*\s*du\s*,", header)
    jl = open(os.path.join(ROOT, "julia", "QuadraticProgramSolverHIP.jl")).read()
    assert re.search(r"ccall\(\(:qps_adjoint_shared,\s*LIBQPS\),\s*Int32,\s*\(Ptr\{Cvoid\},\s*Ptr\{Float64\},\s*Ptr\{Float64\},\s*Ptr\{Float64\},\s*Ref\{QpsParams\},"
                     r"\s*Ptr\{Float64\},\s*Ptr\{Float64\},\s*Ptr\{Float64\},\s*Ptr\{Float64\},\s*Ptr\{Float64\},\s*Ptr\{UInt8\}\)", jl)
    assert hasattr(qps.QuadraticProgramSharedBatch, "adjoint") and qps.QuadraticProgramCgSharedBatch.adjoint is qps.QuadraticProgramSharedBatch.adjoint


def test_null_handle_is_refused_without_a_device(qps):
    from quadraticprogramsolver_amd import _lib
    L = _lib.lib()
    p = _lib.default_params()
    v = np.zeros(4); ptr = v.ctypes.data_as(C.POINTER(C.c_double))
    assert L.qps_adjoint_shared(None, ptr, ptr, ptr, C.byref(p), ptr, ptr, ptr, None, None, None) == BAD_ARGUMENT
    assert L.qps_adjoint_shared(None, None, None, None, None, None, None, None, None, None, None) == BAD_ARGUMENT


def _own_solution(P, A, q, l, u, y):
    """(x, lambda at full length m) of the direct solve of K t = [-q; l_L; u_U] on the active sets of y."""
    Lo, Up = y < 0, y > 0
    act = np.concatenate([np.flatnonzero(Lo), np.flatnonzero(Up)])
    Aa = A[act]
    t = np.linalg.solve(np.block([[P, Aa.T], [Aa, np.zeros((act.size, act.size))]]), np.concatenate([-q, l[Lo], u[Up]]))
    lam = np.zeros(A.shape[0])
    lam[act] = t[P.shape[0]:]
    return t[:P.shape[0]], lam


def test_the_formulas_against_central_differences():
    """d/dh of g'x(theta + h dtheta) for a random direction in q, the finite entries of l and u, symmetric P and A on their patterns, against the six formulas at
    the direct solve's own (x, lambda); the active sets stay those of the thresholded y."""
    h, worst = 1e-5, 0.0
    for name, count in FD_FAMILIES:
        P, A, Q, L, U = polish_cases.family(name, count)
        pat = cases.canonical_pattern(P, A)
        Pj, Aj = cases._columns_of(pat[0]), cases._columns_of(pat[2])
        for b in range(count):
            y = polish_cases.threshold(polish_cases.state(name, b)[1])
            n, m = P.shape[0], A.shape[0]
            g = cases.gx(b, n)
            rng = np.random.default_rng(100 + b)
            dq, dl, du = rng.standard_normal(n), np.where(np.isfinite(L[b]), rng.standard_normal(m), 0.0), np.where(np.isfinite(U[b]), rng.standard_normal(m), 0.0)
            S = rng.standard_normal((n, n))
            dP, dA = np.zeros((n, n)), np.zeros((m, n))
            dP[pat[1], Pj] = (S + S.T)[pat[1], Pj]
            dA[pat[3], Aj] = rng.standard_normal(pat[3].size)
            l0, u0 = np.where(np.isfinite(L[b]), L[b], 0.0), np.where(np.isfinite(U[b]), U[b], 0.0)   # an infinite bound is never active
            loss = lambda s: g @ _own_solution(P + s * dP, A + s * dA, Q[b] + s * dq, l0 + s * dl, u0 + s * du, y)[0]
            fd = (loss(h) - loss(-h)) / (2 * h)
            x, lam = _own_solution(P, A, Q[b], l0, u0, y)
            assert np.all(np.sign(lam[y != 0]) == np.sign(y[y != 0])), (name, b)          # the direct solve's lambda has the sign of y on every active row
            o = cases.outputs(*cases.solve_direct(P, A, y, g), x, lam, pat)
            an = o["dQ"] @ dq + o["dL"] @ dl + o["dU"] @ du + o["vP"] @ dP[pat[1], Pj] + o["vA"] @ dA[pat[3], Aj]
            rel = abs(fd - an) / max(abs(fd), abs(an))
            print(f"{name} column {b}: central difference {fd:.10e} formulas {an:.10e} relative difference {rel:.2e}")
            worst = max(worst, rel)
    assert worst <= 1e-6


def test_an_empty_active_set_gives_the_unconstrained_system():
    for name, count in FD_FAMILIES:
        P, A, _, _, _ = polish_cases.family(name, count)
        n, m = P.shape[0], A.shape[0]
        g, x = cases.gx(0, n), polish_cases.state(name, 0)[0]
        rx, rl = cases.solve_direct(P, A, np.zeros(m), g)
        o = cases.outputs(rx, rl, x, np.zeros(m), cases.canonical_pattern(P, A))
        assert np.abs(rx - np.linalg.solve(P, g)).max() <= 1e-12 * max(1.0, np.abs(rx).max())
        assert not o["dL"].any() and not o["dU"].any() and not o["vA"].any()


def test_the_cap_of_the_flag_test_is_clear_of_every_column():
    counts = cases.first_call_counts()
    print("first-call MINRES counts of the restatement:", counts)
    over = tuple(b for b, c in enumerate(counts) if c > cases.FLAG_CAP)
    assert over == cases.FLAG_COLUMNS_OVER and 0 < len(over) < len(counts)
    assert all(abs(c - cases.FLAG_CAP) >= 0.2 * cases.FLAG_CAP for c in counts)


def test_every_bound_is_recorded_for_every_output():
    assert set(cases.BOUNDS) == set(cases.MEASURED)
    assert all(set(v) == set(cases.OUTPUTS) and all(0 <= x < 1e-5 for x in v.values()) for v in cases.BOUNDS.values())


def test_row_of_entry_builder_under_asan_and_ubsan(tmp_path):
    """csc_column_of_entry of spmv_layout.cpp on the patterns of P and A of the sparse cases, in a stand-alone program."""
    exe, patterns = tmp_path / "entry_column_check", tmp_path / "patterns.txt"
    src = [os.path.join(ROOT, "tests", "capi", "entry_column_check.cpp"), os.path.join(ROOT, "quadraticprogramsolver_amd", "csrc", "spmv_layout.cpp")]
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-static-libasan", "-static-libubsan",          # the runtimes in the program itself: nothing about it depends on the load order
                            "-Wall", "-Wextra", "-o", str(exe)] + src, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    count = 0
    with open(patterns, "w") as f:
        for name in ("random", "banded", "banded71"):
            (P, A, _, _, _), _, _ = cases.case(name, 3)
            pat = cases.canonical_pattern(P, A)
            for cp in (pat[0], pat[2]):
                f.write(f"{cp.size - 1} {cp[-1]}\n{' '.join(map(str, cp))}\n")
                count += 1
        f.write("3 0\n0 0 0 0\n")                                           # an empty matrix
        f.write("4 5\n0 2 2 4 5\n")                                         # an empty column 1
        f.write("3 3\n0 0 0 3\n")                                           # empty leading columns
        count += 3
    res = subprocess.run([str(exe), str(patterns)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(res.stdout)
    assert res.returncode == 0, res.stdout
    assert f"{count} patterns" in res.stdout
