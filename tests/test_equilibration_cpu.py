"""CPU-only checks of the opt-in Ruiz equilibration of the shared-matrix batches (qps_set_shared_equilibration): both symbols are declared, exported and bound in
header, library, ctypes and Julia; a NULL handle and a bad pass count are refused without a device; and every case the GPU tests of
tests/test_gpu_equilibration.py use passes its guard in the numpy restatement of tests/equilibration_cases.py -- the reduced and the KKT form take the same
decisions and agree at the fixed K to a tenth of the device bound, no decision of the family-wide rho rule sits on a rounding edge, and the families do what the
tests say they do (the scrambled family needs the scaling, the spread-4 family reaches both clamps).  The step of one pass as the library computes it
(equil_step of csrc/shared_family_rules.h, through the host-test shim) is the restated integer rule."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import equilibration_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARGUMENT = 1
SCRAMBLED = ("scrambled", 96, 160, 4)
SPARSE = ("random", 20)
FCTR_RHO = 4.0          # the family-rho composition case: at 5 a quotient passes within 4.7 % of the threshold, at 4 the closest is 15 % away


def test_symbols_are_declared_exported_and_bound(qps):
    from quadraticprogramsolver_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qps.h")).read(), flags=re.S)
    assert re.search(r"\bint32_t\s+qps_set_shared_equilibration\s*\(\s*qps_handle\s+\w+\s*,\s*int32_t\s+\w+\s*\)", header)
    assert re.search(r"\bint32_t\s+qps_get_shared_equilibration\s*\(\s*qps_handle\s+\w+\s*,\s*double\s*\*\s*\w+\s*,\s*double\s*\*\s*\w+\s*\)", header)
    jl = re.sub(r"#[^\n]*", "", open(os.path.join(ROOT, "julia", "QuadraticProgramSolverHIP.jl"), encoding="utf-8").read())
    assert re.search(r"ccall\(\(:qps_set_shared_equilibration,\s*LIBQPS\),\s*Int32,\s*\(Ptr\{Cvoid\},\s*Int32\)", jl)
    assert re.search(r"ccall\(\(:qps_get_shared_equilibration,\s*LIBQPS\),\s*Int32,\s*\(Ptr\{Cvoid\},\s*Ptr\{Float64\},\s*Ptr\{Float64\}\)", jl)
    raw = C.CDLL(_lib.LIB_PATH)
    for name, args in (("qps_set_shared_equilibration", [C.c_void_p, C.c_int32]),
                       ("qps_get_shared_equilibration", [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)])):
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(raw, name), f"{name} is not exported by the library"
        fn = getattr(_lib.lib(), name)
        assert fn.restype is C.c_int32 and list(fn.argtypes) == args
    for cls in (qps.QuadraticProgramSharedBatch, qps.QuadraticProgramSparseSharedBatch):
        assert hasattr(cls, "set_equilibration") and hasattr(cls, "equilibration")


def test_null_handle_and_bad_passes_are_refused_without_a_device(qps):
    from quadraticprogramsolver_amd import _lib
    L = _lib.lib()
    for passes in (10, 0, 51, -1):
        assert L.qps_set_shared_equilibration(None, passes) == BAD_ARGUMENT
    assert b"NULL" in L.qps_last_error(None)
    assert L.qps_get_shared_equilibration(None, None, None) == BAD_ARGUMENT


def test_the_rule_on_a_matrix_worked_by_hand():
    """P = diag(16, 1/64), A = [[4, 0], [0, 0]].  Pass 1: cn = (16, 1/64) = (0.5 2^5, 0.5 2^-5) gives steps -floor(5 / 2) = -2 and -floor(-5 / 2) = +3;
    rn = (4, 0) = (0.5 2^3, 0) gives -1 and, for the empty row, 0.  Pass 2 reads P~ = diag(1, 1) and A~_00 = 4 2^(-1 - 2) = 0.5: 1 = 0.5 2^1 and 0.5 = 0.5 2^0
    both give step 0, so the exponents stay."""
    P, A = np.diag([16.0, 1.0 / 64.0]), np.array([[4.0, 0.0], [0.0, 0.0]])
    kd, ke = ec.ruiz_pow2(P, A, 1)
    assert kd.tolist() == [-2, 3] and ke.tolist() == [-1, 0]
    kd2, ke2 = ec.ruiz_pow2(P, A, 2)
    assert kd2.tolist() == [-2, 3] and ke2.tolist() == [-1, 0]
    assert ec.ruiz_pow2(P, A, 0)[0].tolist() == [0, 0]


STEP_INPUTS = [0.0, -3.0, 1.0, 0.5, 2.0, 4.0, 3.0, 2.0 ** -1021, 5e-324, 1e308]
#   v = f 2^e, f in [0.5, 1):  -   -    e=1  e=0  e=2  e=3  e=2  e=-1020      e=-1073 e=1024
STEP_BY_HAND = [0, 0, 0, 0, -1, -1, -1, 510, 537, -512]


def test_the_library_step_is_the_restated_integer_rule():
    """-floor(e / 2) with floor towards minus infinity (e = 1 gives 0, e = -1073 gives +537), 0 for a norm that is not positive; the clamp is the restatement's."""
    from host_shim import rules
    clamp = C.c_int(0)
    got = [rules().lt_equil_step(v, C.byref(clamp)) for v in STEP_INPUTS]
    want = [int(k) for k in ec._step(np.array(STEP_INPUTS))]
    print("v", STEP_INPUTS, "library", got, "restatement", want)
    assert got == want == STEP_BY_HAND
    assert clamp.value == ec.K_CLAMP


def test_fp32_handles_scale_the_rounded_matrices():
    """2 (1 - 2^-30) is 0.99.. 2^1 in double (step 0) and rounds to 2.0 = 0.5 2^2 in fp32 (step -1): the norms come from the entries as the handle stores them."""
    v = 2.0 * (1.0 - 2.0 ** -30)
    P, A = np.diag([v, 1.0]), np.array([[1.0, 0.0]])
    assert ec.ruiz_pow2(P, A, 1, "f64")[0].tolist() == [0, 0]
    assert ec.ruiz_pow2(P, A, 1, "f32")[0].tolist() == [-1, 0]


def test_the_scrambled_family_needs_the_scaling_and_stops_where_the_issue_says():
    for form in ("reduced", "kkt"):
        on = ec.run(SCRAMBLED, form)["columns"]
        assert [c["iterations"] for c in on] == [950, 100, 125, 75] and [c["convFlag"] for c in on] == [3, 3, 3, 3], form
    off = ec.run(SCRAMBLED, "reduced", passes=0)["columns"]
    assert [c["iterations"] for c in off] == [5000] * 4 and [c["convFlag"] for c in off] == [1] * 4


def test_the_spread_four_family_reaches_both_clamps():
    P, A, _, _, _ = ec.family("scrambled", 200, 330, 4, 4.0)
    for dtype in ("f64", "f32"):
        kd, ke = ec.ruiz_pow2(P, A, ec.PASSES, dtype)
        k = np.concatenate([kd, ke])
        print(dtype, "kd", kd.min(), kd.max(), "ke", ke.min(), ke.max())
        assert k.min() == -ec.K_CLAMP and k.max() == ec.K_CLAMP


def _rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.mark.parametrize("key,K", [(SCRAMBLED, 100), (SPARSE, 100)], ids=["scrambled96", "random20"])
def test_the_two_forms_agree_at_the_fixed_k(key, K):
    """A tenth of the device bound (1e-9 on x and z, 1e-8 on y), with the warm start the GPU tests use."""
    kw = dict(numIterations=K, epsAbs=0.0, epsRel=0.0, warm=True)
    red, kkt = ec.run(key, "reduced", **kw), ec.run(key, "kkt", **kw)
    worst = [max(_rel(a[q], b[q]) for a, b in zip(red["columns"], kkt["columns"])) for q in "xzy"]
    print(key, "reduced against kkt at K =", K, "rel x z y:", [f"{w:.1e}" for w in worst])
    assert worst[0] <= 1e-10 and worst[1] <= 1e-10 and worst[2] <= 1e-9


@pytest.mark.parametrize("key,kind", [(SCRAMBLED, None), (SCRAMBLED, "equality"), (SPARSE, None)], ids=["scrambled96", "scrambled96-equality", "random20"])
def test_the_two_forms_stop_at_the_same_iteration(key, kind):
    red, kkt = ec.run(key, "reduced", kind=kind)["columns"], ec.run(key, "kkt", kind=kind)["columns"]
    print(key, kind, [(c["iterations"], c["convFlag"]) for c in red])
    assert [(c["iterations"], c["convFlag"]) for c in red] == [(c["iterations"], c["convFlag"]) for c in kkt]
    assert all(c["convFlag"] != 1 for c in red)


def test_family_rho_case_guard():
    """As tests/test_family_rho_cpu.py demands: same switches, flags and stopping iterations in both forms, every proposal at least 2 % away from fctrRho and
    1 / fctrRho, and the switched rho of the two forms within a tenth of the 1e-10 the device is held to."""
    red, kkt = (ec.run(SCRAMBLED, form, adaptive=True, fctrRho=FCTR_RHO) for form in ("reduced", "kkt"))
    for r in (red, kkt):
        edge = min(min(abs(q / FCTR_RHO - 1.0), abs(q * FCTR_RHO - 1.0)) for _, q in r["quotients"])
        print("switches", [(s[0], s[2]) for s in r["switches"]], "closest quotient:", f"{edge:.3f}")
        assert edge >= 0.02
        assert [s[0] for s in r["switches"]] == [26]
    assert [(c["iterations"], c["convFlag"], c["numRefactor"]) for c in red["columns"]] == [(c["iterations"], c["convFlag"], c["numRefactor"]) for c in kkt["columns"]]
    assert [i for i, _ in red["quotients"]] == [i for i, _ in kkt["quotients"]]
    spread = [abs(a - b) / b for (_, _, a), (_, _, b) in zip(red["switches"], kkt["switches"])]
    print("new rho, reduced against kkt, relative:", [f"{v:.1e}" for v in spread])
    assert max(spread) <= 1e-11


def test_passes_zero_is_the_unscaled_restatement():
    from family_rho_cases import FamilyRestatement
    P, A, Q, L, U = ec.family(*SCRAMBLED)
    ref = FamilyRestatement(P, A, form="reduced").solve(Q, L, U, adaptive=False, numIterations=50, epsAbs=0.0, epsRel=0.0)
    r = ec.run(SCRAMBLED, "reduced", passes=0, numIterations=50, epsAbs=0.0, epsRel=0.0)
    for a, b in zip(r["columns"], ref["columns"]):
        assert np.array_equal(a["x"], b["x"]) and np.array_equal(a["y"], b["y"])


def test_the_out_of_range_family_leaves_fp32_and_stays_inside_fp64():
    P, A, _, _, _ = ec.out_of_range_family()
    kd, ke = ec.ruiz_pow2(P, A, ec.PASSES, "f32")
    S = np.abs(A.astype(np.float32).astype(np.float64)) * np.ldexp(1.0, ke)[:, None] * np.ldexp(1.0, kd)[None, :]
    assert S[S > 0].min() < np.finfo(np.float32).tiny
    assert np.float32(A[0, 0]) >= np.finfo(np.float32).tiny          # a normal fp32 number before the scaling
    assert S[S > 0].min() > np.finfo(np.float64).tiny
