"""Opt-in Ruiz equilibration of the shared-matrix batches on the device (qps_set_shared_equilibration): the scale vectors equal the integer rule of
tests/equilibration_cases.py exactly, and every column behaves as the numpy restatement there -- the loop on the scaled data, the check on the unscaled iterates --
in its reduced Cholesky form for the dense handle and its dense KKT form for the sparse one.  rho = 0.1, 10 passes unless a test says otherwise.

Bounds are the project's for these families (tests/test_gpu_rho_scale.py): fp64 1e-9 relative on x and z, 1e-8 on y, residuals as there; fp32 1e-3.  The two
forms of the restatement agree among themselves to 4.1e-14 on these cases (tests/test_equilibration_cpu.py holds them to a tenth of the bounds)."""
import ctypes as C

import numpy as np
import pytest

import equilibration_cases as ec
from equilibration_cases import PASSES, RHO, ruiz_pow2, warm_start
from test_gpu_parity import rel

pytestmark = pytest.mark.gpu

UNSUPPORTED = 8
SCRAMBLED = ("scrambled", 96, 160, 4)          # cached kernel form: n and m no multiples of 64, count no multiple of 16
CLAMPED = ("scrambled", 200, 330, 4, 4.0)      # spread 4: exponents at both clamps
STAGED = ("scrambled", 2112, 2304, 37)         # matrix above 32 MiB: staged kernel form, two panels per workgroup plus a ragged one
SPARSE = ("random", 20)                        # n = 100, m = 50, two panels
FCTR_RHO = 4.0                                 # tests/test_equilibration_cpu.py: every proposal stays 15 % clear of the thresholds


def _make(gpu, sparse, P, A, Q, L, U, **kw):
    return (gpu.QuadraticProgramSparseSharedBatch if sparse else gpu.QuadraticProgramSharedBatch)(P, A, Q, L, U, **kw)


def _run(prob, mX=None, **kw):
    X, flags, infos = prob.solve(mX, **kw)
    Z, Y = prob.dual()
    return X, Z, Y, [int(f) for f in flags], infos


def _same(a, b):
    keys = ("iterations", "numRefactor", "rhoFinal", "rhoProposed", "resPrim", "resDual")
    return (all(np.array_equal(p, q) for p, q in zip(a[:3], b[:3])) and a[3] == b[3]
            and all(np.array_equal(i[k], j[k], equal_nan=True) for i, j in zip(a[4], b[4]) for k in keys))


# ---------------------------------------------------------------------------------------------------------------------
# 1. scale vectors
# ---------------------------------------------------------------------------------------------------------------------
VECTORS = [(SCRAMBLED, 1, False), (SCRAMBLED, 10, False), (CLAMPED, 10, False), (STAGED, 10, False), (SPARSE, 1, True), (SPARSE, 10, True)]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("key,passes,sparse", VECTORS, ids=[f"{'x'.join(map(str, k))}-p{p}" for k, p, _ in VECTORS])
def test_scale_vectors_equal_the_integer_rule(gpu, key, passes, sparse, dtype):
    P, A, Q, L, U = ec.family(*key)
    kd, ke = ruiz_pow2(P, A, passes, dtype)
    with _make(gpu, sparse, P, A, Q, L, U, dtype=dtype) as prob:
        vD, vE = prob.equilibration()
        assert np.array_equal(vD, np.ones(P.shape[0])) and np.array_equal(vE, np.ones(A.shape[0]))      # all ones while off
        prob.set_equilibration(passes)
        vD, vE = prob.equilibration()
        print(f"{key} {dtype} passes {passes}: kd {kd.min()}..{kd.max()} ke {ke.min()}..{ke.max()}; mismatches D {(vD != 2.0 ** kd).sum()} E {(vE != 2.0 ** ke).sum()}")
        assert np.array_equal(vD, 2.0 ** kd) and np.array_equal(vE, 2.0 ** ke)
        prob.set_equilibration(None)
        vD, vE = prob.equilibration()
        assert np.array_equal(vD, np.ones(P.shape[0])) and np.array_equal(vE, np.ones(A.shape[0]))
    if key == CLAMPED:
        assert min(kd.min(), ke.min()) == -13 and max(kd.max(), ke.max()) == 13


# ---------------------------------------------------------------------------------------------------------------------
# 2. parity per column at a fixed K, non-zero warm start
# ---------------------------------------------------------------------------------------------------------------------
FIXED = [(SCRAMBLED, 100, False, range(4)), (STAGED, 60, False, (0, 15, 16, 31, 32, 36)), (SPARSE, 100, True, range(20))]


@pytest.mark.parametrize("key,K,sparse,cols", FIXED, ids=["x".join(map(str, k)) for k, _, _, _ in FIXED])
def test_fixed_k_iterates_match_the_restatement_per_column(gpu, key, K, sparse, cols):
    P, A, Q, L, U = ec.family(*key)
    ref = ec.run(key, "kkt" if sparse else "reduced", numIterations=K, epsAbs=0.0, epsRel=0.0, warm=True)["columns"]
    with _make(gpu, sparse, P, A, Q, L, U) as prob:
        prob.set_equilibration(PASSES)
        X, Z, Y, flags, infos = _run(prob, warm_start(Q), numIterations=K, ϵAbs=0.0, ϵRel=0.0, ρ=RHO)
    for b in cols:
        r = ref[b]
        fig = (rel(X[b], r["x"]), rel(Z[b], r["z"]), rel(Y[b], r["y"]), abs(infos[b]["resPrim"] - r["resPrim"]) / max(1.0, r["resPrim"]),
               abs(infos[b]["resDual"] - r["resDual"]) / max(1.0, r["resDual"]))
        print(f"{key} column {b}: rel x {fig[0]:.2e} z {fig[1]:.2e} y {fig[2]:.2e} dresPrim {fig[3]:.2e} dresDual {fig[4]:.2e}")
        assert flags[b] == 1 and infos[b]["iterations"] == K
        assert infos[b]["rhoFinal"] == RHO and infos[b]["rhoProposed"] == RHO
        assert fig[0] <= 1e-9 and fig[1] <= 1e-9 and fig[2] <= 1e-8
        assert fig[3] <= 1e-9 and fig[4] <= 1e-9
        assert np.all(L[b] <= Z[b]) and np.all(Z[b] <= U[b])          # qps_get_dual returns the unscaled z: inside the caller's bounds


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
def test_fp32(gpu, sparse):
    key = SPARSE if sparse else SCRAMBLED
    P, A, Q, L, U = ec.family(*key)
    ref = ec.run(key, "kkt" if sparse else "reduced", numIterations=100, epsAbs=0.0, epsRel=0.0, warm=True, dtype="f32")["columns"]
    with _make(gpu, sparse, P, A, Q, L, U, dtype="f32") as prob:
        prob.set_equilibration(PASSES)
        X, _, infos = prob.solve(warm_start(Q), numIterations=100, ϵAbs=0.0, ϵRel=0.0, ρ=RHO)
    for b in range(Q.shape[0]):
        print(f"fp32 {key} column {b}: rel x at K = 100 {rel(X[b], ref[b]['x']):.2e}")
        assert infos[b]["iterations"] == 100 and rel(X[b], ref[b]["x"]) <= 1e-3


# ---------------------------------------------------------------------------------------------------------------------
# 3. to eps = 1e-6
# ---------------------------------------------------------------------------------------------------------------------
def test_every_column_stops_where_the_restatement_stops_and_none_without_the_scaling(gpu):
    P, A, Q, L, U = ec.family(*SCRAMBLED)
    ref = ec.run(SCRAMBLED, "reduced")["columns"]
    with gpu.QuadraticProgramSharedBatch(P, A, Q, L, U) as prob:
        _, flags_off, infos_off = prob.solve(numIterations=1000, ϵAbs=1e-6, ϵRel=1e-6, ρ=RHO)
        prob.set_equilibration(PASSES)
        _, flags, infos = prob.solve(numIterations=1000, ϵAbs=1e-6, ϵRel=1e-6, ρ=RHO)
    print("on:", [(int(f), i["iterations"]) for f, i in zip(flags, infos)], "off:", [(int(f), i["iterations"]) for f, i in zip(flags_off, infos_off)])
    assert [int(f) for f in flags] == [c["convFlag"] for c in ref] == [3, 3, 3, 3]
    assert [i["iterations"] for i in infos] == [c["iterations"] for c in ref] == [950, 100, 125, 75]
    assert [int(f) for f in flags_off] == [1] * 4 and [i["iterations"] for i in infos_off] == [1000] * 4


# ---------------------------------------------------------------------------------------------------------------------
# 4. composition
# ---------------------------------------------------------------------------------------------------------------------
def test_with_the_equality_rho_scale(gpu):
    P, A, Q, L, U = ec.family(*SCRAMBLED)
    ref = ec.run(SCRAMBLED, "reduced", kind="equality")["columns"]
    with gpu.QuadraticProgramSharedBatch(P, A, Q, L, U) as prob:
        prob.set_rho_scale(gpu.equality_rho_scale(L, U))
        prob.set_equilibration(PASSES)                                 # set after the rho scale: diag(sqrt(s)) A is rebuilt from the scaled A
        _, flags, infos = prob.solve(numIterations=5000, ϵAbs=1e-6, ϵRel=1e-6, ρ=RHO)
    print([(int(f), i["iterations"]) for f, i in zip(flags, infos)], [(c["convFlag"], c["iterations"]) for c in ref])
    assert [int(f) for f in flags] == [c["convFlag"] for c in ref] and [i["iterations"] for i in infos] == [c["iterations"] for c in ref]


def test_with_the_family_wide_rho_rule(gpu):
    """The base rho moves by the rule on the UNSCALED norms."""
    P, A, Q, L, U = ec.family(*SCRAMBLED)
    ref = ec.run(SCRAMBLED, "reduced", adaptive=True, fctrRho=FCTR_RHO)
    with gpu.QuadraticProgramSharedBatch(P, A, Q, L, U) as prob:
        prob.set_equilibration(PASSES)
        prob.set_adaptive_rho()
        _, flags, infos = prob.solve(numIterations=5000, ϵAbs=1e-6, ϵRel=1e-6, ρ=RHO, fctrΡ=FCTR_RHO)
    for b, c in enumerate(ref["columns"]):
        d = abs(infos[b]["rhoFinal"] - c["rhoFinal"]) / c["rhoFinal"]
        print(f"column {b}: flag {int(flags[b])}/{c['convFlag']} iterations {infos[b]['iterations']}/{c['iterations']} numRefactor {infos[b]['numRefactor']}/{c['numRefactor']} "
              f"rhoFinal {infos[b]['rhoFinal']!r} rel {d:.1e}")
        assert int(flags[b]) == c["convFlag"] and infos[b]["iterations"] == c["iterations"] and infos[b]["numRefactor"] == c["numRefactor"]
        assert d <= 1e-10
    assert len(ref["switches"]) == 1


# ---------------------------------------------------------------------------------------------------------------------
# 5. bit-for-bit identities
# ---------------------------------------------------------------------------------------------------------------------
KW = dict(numIterations=150, ϵAbs=1e-4, ϵRel=1e-4, ρ=RHO)


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
def test_identities_bit_for_bit(gpu, sparse):
    key = SPARSE if sparse else SCRAMBLED
    P, A, Q, L, U = ec.family(*key)
    X0 = warm_start(Q)
    Q2 = Q[::-1].copy()
    with _make(gpu, sparse, P, A, Q, L, U) as prob:
        never = _run(prob, X0, **KW)
        prob.set_equilibration(PASSES)
        on = _run(prob, X0, **KW)
        again = _run(prob, X0, reuseFactor=True, **KW)
        prob.set_equilibration(0)
        off = _run(prob, X0, reuseFactor=True, **KW)
        prob.set_equilibration(3)
        other = _run(prob, X0, **KW)
        prob.set_equilibration(PASSES)                                 # re-set with another pass count: through the unscaled matrices
        on2 = _run(prob, X0, reuseFactor=True, **KW)
        prob.update(mQ=Q2)
        upd = _run(prob, X0, reuseFactor=True, **KW)
    assert _same(again, on), "run equals run"
    assert _same(off, never), "off after on equals a handle that never saw the call"
    assert _same(on2, on), "on - off - on equals a fresh handle with the option on"
    assert not np.array_equal(on[0], never[0]) and not np.array_equal(other[0], on[0])
    with _make(gpu, sparse, P, A, Q, L, U) as fresh:
        fresh.set_equilibration(PASSES)
        assert _same(_run(fresh, X0, **KW), on2)
    with _make(gpu, sparse, P, A, Q2, L, U) as fresh:
        fresh.set_equilibration(PASSES)
        assert _same(_run(fresh, X0, **KW), upd), "update after setting equals a fresh handle created with those vectors"
    for b in (0, Q.shape[0] - 1):
        with _make(gpu, sparse, P, A, Q[b:b + 1], L[b:b + 1], U[b:b + 1]) as one:
            one.set_equilibration(PASSES)
            x1, z1, y1, f1, i1 = _run(one, X0[b:b + 1], **KW)
        assert f1[0] == on[3][b] and i1[0]["iterations"] == on[4][b]["iterations"]
        assert np.array_equal(x1[0], on[0][b]) and np.array_equal(z1[0], on[1][b]) and np.array_equal(y1[0], on[2][b]), b


# ---------------------------------------------------------------------------------------------------------------------
# 6. factor bookkeeping
# ---------------------------------------------------------------------------------------------------------------------
def _launches(prob, word):
    hit = [k for k in prob.kernel_times() if word in k["name"]]      # (a category without a sample is not listed)
    assert len(hit) <= 1
    return hit[0]["launches"] if hit else 0


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
def test_setting_and_clearing_invalidate_the_factor_once(gpu, sparse):
    key = SPARSE if sparse else SCRAMBLED
    P, A, Q, L, U = ec.family(*key)
    kw = dict(numIterations=25, ϵAbs=0.0, ϵRel=0.0, ρ=RHO, reuseFactor=True)
    with _make(gpu, sparse, P, A, Q, L, U) as prob:
        prob.solve(**kw)
        for passes in (PASSES, 0):
            prob.set_equilibration(passes)
            prob.set_profiling(1)
            prob.solve(**kw)
            assert _launches(prob, "factorisation at setup") == 1, passes
            prob.set_profiling(1)                                      # clears the counts
            prob.solve(**kw)
            assert _launches(prob, "factorisation at setup") == 0, passes


# ---------------------------------------------------------------------------------------------------------------------
# 7. refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_other_handles_are_unsupported(gpu):
    from quadraticprogramsolver_amd import _lib
    L_ = _lib.lib()
    P, A, Q, L, U = ec.family(*SCRAMBLED)
    n, m = P.shape[0], A.shape[0]
    vD, vE = np.zeros(n), np.zeros(m)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    with gpu.QuadraticProgram(P, Q[0], A, L[0], U[0]) as one, gpu.QuadraticProgramBatch([(P, Q[b], A, L[b], U[b]) for b in range(2)]) as batch, \
            gpu.ProxQP(P, Q[0], A[:8], np.zeros(8), A[8:], U[0][8:]) as prox:
        for h in (one._h, batch._h, prox._h):
            assert L_.qps_set_shared_equilibration(h, 10) == UNSUPPORTED
            assert b"shared-matrix batch" in L_.qps_last_error(h)
            assert L_.qps_set_shared_equilibration(h, 0) == UNSUPPORTED
            assert L_.qps_get_shared_equilibration(h, dp(vD), dp(vE)) == UNSUPPORTED
            assert L_.qps_set_shared_equilibration(h, 51) == 1          # the argument is judged first


def test_an_entry_that_would_leave_the_normal_range_is_refused(gpu):
    P, A, Q, L, U = ec.out_of_range_family()
    kw = dict(numIterations=50, ϵAbs=0.0, ϵRel=0.0, ρ=RHO)
    with gpu.QuadraticProgramSharedBatch(P, A, Q, L, U, dtype="f32") as prob:
        plain = _run(prob, **kw)
        with pytest.raises(gpu.QpsError) as e:
            prob.set_equilibration(PASSES)
        assert e.value.status == UNSUPPORTED and "normal range" in e.value.message
        vD, vE = prob.equilibration()
        assert np.array_equal(vD, np.ones(4)) and np.array_equal(vE, np.ones(4))
        assert _same(_run(prob, reuseFactor=True, **kw), plain)          # the handle solves as before
        with pytest.raises(gpu.QpsError) as e:
            prob.set_equilibration(51)
        assert e.value.status == 1
        with pytest.raises(gpu.QpsError) as e:
            prob.solve(adptΡ=True, **kw)
        assert e.value.status == UNSUPPORTED
    with gpu.QuadraticProgramSharedBatch(P, A, Q, L, U) as prob:          # fp64 holds the same entry easily
        prob.set_equilibration(PASSES)
        kd, ke = ruiz_pow2(P, A, PASSES)
        assert np.array_equal(prob.equilibration()[0], 2.0 ** kd)
