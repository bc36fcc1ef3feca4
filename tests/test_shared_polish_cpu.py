"""CPU-only guards of the polishing step on the shared-matrix batches (qps_polish_shared, qps_set_shared_polish): the bindings, the refusals that need no device,
and the properties of the cases that tests/test_gpu_shared_polish.py relies on -- without them the GPU tests prove less.  No device is used."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import shared_polish_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARGUMENT = 1


def _read(*parts):
    with open(os.path.join(ROOT, *parts), encoding="utf-8") as f:
        return f.read()


def test_header_julia_and_ctypes_bind_both_entry_points(qps):
    from quadraticprogramsolver_amd import _lib
    header = _read("include", "qps.h")
    assert re.search(r"\bint32_t\s+qps_polish_shared\s*\(\s*qps_handle\s+\w+\s*,\s*double\s*\*\s*\w+\s*,\s*const\s+double\s*\*\s*\w+\s*,\s*const\s+qps_params\s*\*\s*\w+\s*,"
                     r"\s*qps_polish_report\s*\*\s*\w+\s*\)\s*;", header)
    assert re.search(r"\bint32_t\s+qps_set_shared_polish\s*\(\s*qps_handle\s+\w+\s*,\s*int32_t\s+\w+\s*(/\*.*?\*/)?\s*\)\s*;", header)
    assert "scaled variables" in header                                   # what delta and epsMinres mean under the equilibration
    jl = _read("julia", "QuadraticProgramSolverHIP.jl")
    assert re.search(r"ccall\(\(:qps_polish_shared,\s*LIBQPS\),\s*Int32,\s*\(Ptr\{Cvoid\},\s*Ptr\{Float64\},\s*Ptr\{Float64\},\s*Ref\{QpsParams\},\s*Ptr\{UInt8\}\)", jl)
    assert re.search(r"ccall\(\(:qps_set_shared_polish,\s*LIBQPS\),\s*Int32,\s*\(Ptr\{Cvoid\},\s*Int32\)", jl)
    L = _lib.lib()
    dp = C.POINTER(C.c_double)
    assert list(L.qps_polish_shared.argtypes) == [C.c_void_p, dp, dp, C.POINTER(_lib.QpsParams), C.POINTER(_lib.QpsPolishReport)] and L.qps_polish_shared.restype is C.c_int32
    assert list(L.qps_set_shared_polish.argtypes) == [C.c_void_p, C.c_int32] and L.qps_set_shared_polish.restype is C.c_int32
    assert {"qps_polish_shared", "qps_set_shared_polish"} <= set(_lib.EXPORTED_SYMBOLS)
    for cls in (qps.QuadraticProgramSharedBatch, qps.QuadraticProgramSparseSharedBatch):
        assert callable(cls.polish) and callable(cls.set_polish)
    assert qps.QuadraticProgramSparseSharedBatch.polish is qps.QuadraticProgramSharedBatch.polish      # inherited, not restated


def test_a_null_handle_is_a_bad_argument_without_a_device(qps):
    from quadraticprogramsolver_amd import _lib
    L = _lib.lib()
    x = np.zeros(4); p = _lib.default_params(); rep = _lib.QpsPolishReport()
    ptr = x.ctypes.data_as(C.POINTER(C.c_double))
    assert L.qps_polish_shared(None, ptr, ptr, C.byref(p), C.byref(rep)) == BAD_ARGUMENT
    assert L.qps_polish_shared(None, None, None, None, None) == BAD_ARGUMENT
    assert L.qps_set_shared_polish(None, 1) == BAD_ARGUMENT and L.qps_set_shared_polish(None, 0) == BAD_ARGUMENT


PARITY_IDS = [("dense", b) for b in sorted({b for cols in cases.PARITY_COLUMNS.values() for b in cols})] + [("random", b) for b in (0, 1, 2, 15, 16, 19)]


@pytest.mark.parametrize("name,b", PARITY_IDS)
def test_the_restatement_is_a_reference_on_every_compared_column(name, b):
    """Flag 0 with 10 refinements, no |y| within a decade of the threshold, within 1e-9 of the direct solve, and the ADMM x more than 1e-6 from it: a polish that
    does nothing is visible."""
    x, y = cases.state(name, b)
    xr, flag, info = cases.restatement(name, b)
    t = cases.direct_of(name, b)
    assert flag == 0 and info["refinements"] == 10
    assert not np.any((np.abs(y) >= cases.Y_THRESHOLD / 10) & (np.abs(y) <= cases.Y_THRESHOLD * 10))
    assert np.abs(xr - t).max() <= 1e-9
    assert np.abs(x - t).max() > 1e-6


@pytest.mark.parametrize("name,count", [("dense", 37), ("random", 37)])
def test_no_multiplier_of_a_family_lies_near_the_threshold(name, count):
    """Every column of the device tests goes through the threshold (the direct solve is compared on all of them)."""
    for b in range(count):
        y = cases.state(name, b)[1]
        assert not np.any((np.abs(y) >= cases.Y_THRESHOLD / 10) & (np.abs(y) <= cases.Y_THRESHOLD * 10)), b


def test_first_call_counts_stand_clear_of_the_cap_of_the_flag_test():
    """shared_family(96, 160, 20), numItrPolish = 1, epsMinres = 1e-9: columns 0 and 2 need more than the cap of 500, every other column less, and the nearest
    counts on either side are more than 10 % away from it -- the device's MINRES may stop a few iterations apart from the restatement's, not fifty."""
    its = [cases.first_call_iterations("dense", b) for b in range(20)]
    over = [b for b in range(20) if its[b] > cases.FLAG_CAP]
    assert tuple(over) == cases.FLAG_COLUMNS_OVER
    assert min(its[b] for b in over) > 1.1 * cases.FLAG_CAP
    assert max(its[b] for b in range(20) if b not in over) < 0.9 * cases.FLAG_CAP
    assert min(its) > 2                                                    # numItrMinres = 2 stops every column


def test_the_scaled_restatement_converges_on_the_equilibration_case():
    (P, A, Q, L, U), D, E = cases.equilibrated()
    X, Y = cases.states("scrambled", 4)
    for b in range(4):
        xr, flag, info = cases.equilibrated_restatement(b, D, E, X, Y, 4000)
        assert flag == 0 and info["refinements"] == 10, b
        assert np.abs(xr - cases.direct_of("scrambled", b)).max() <= 1e-9 * max(1.0, np.abs(xr).max())


def test_the_staged_family_is_past_the_cached_form_and_its_figures_are_recorded():
    k = cases.STAGED
    assert 8 * k["n"] * k["m"] > 32 << 20 and k["count"] > 32          # A and A' above the 32 MiB cut; three panels: a pair and a single
    assert k["n"] % 64 == 0 and k["m"] % 64 == 0
    for b in k["columns"]:
        its, d_r, d_admm = cases.STAGED_RESTATEMENT[b]
        assert 0 < its < 12000 and 4 * d_r < d_admm / 4                   # the two requirements of the device test can hold together
