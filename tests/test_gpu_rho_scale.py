"""Per-constraint rho scale of the shared-matrix batches on the device (qps_set_shared_rho_scale): with a scale vector s shared by all columns, row i runs
with rho_i = rho s_i and every column behaves as the numpy restatement of tests/rho_scale_cases.py on (P, q_b, A, l_b, u_b) -- its reduced Cholesky form
for the dense handle, its dense KKT form for the sparse one.  Base rho = 0.1 throughout.

Bounds are those tests/test_gpu_shared_batch.py and tests/test_gpu_sparse_shared_batch.py use for the same families: dense fp64 and sparse random 1e-9
relative on x and z, 1e-8 on y, residuals as there; lasso 1e-6 / 1e-5; fp32 1e-3."""
import ctypes as C
import functools

import numpy as np
import pytest

from rho_scale_cases import Restatement, scale_of
from shared_batch_cases import shared_family
from sparse_shared_cases import lasso_path, random_family
from test_gpu_parity import ABS_DEV_THR, rel

pytestmark = pytest.mark.gpu

BAD_ARGUMENT, UNSUPPORTED = 1, 8
RHO = 0.1


@functools.lru_cache(maxsize=None)
def family(name, *shape):
    return {"shared": shared_family, "lasso": lasso_path, "random": random_family}[name](*shape)


@functools.lru_cache(maxsize=None)
def restatement(key, kind, form):
    """One factorised restatement per (family, scale, form), shared by the tests of this module."""
    P, A, Q, L, U = family(*key)
    return Restatement(P, A, scale_of(kind, L, U), form=form, rho=RHO)


_REF = {}


def reference(key, kind, form, b, **kw):
    k = (key, kind, form, b, tuple(sorted(kw.items())))
    if k not in _REF:
        P, A, Q, L, U = family(*key)
        _REF[k] = restatement(key, kind, form).solve(Q[b], L[b], U[b], **kw)
    return _REF[k]


def fixed_k_figures(X, Z, Y, infos, b, ref):
    return (rel(X[b], ref["x"]), rel(Z[b], ref["z"]), rel(Y[b], ref["y"]), abs(infos[b]["resPrim"] - ref["resPrim"]) / max(1.0, ref["resPrim"]),
            abs(infos[b]["resDual"] - ref["resDual"]) / max(1.0, ref["resDual"]))


# ---------------------------------------------------------------------------------------------------------------------
# dense handle
# ---------------------------------------------------------------------------------------------------------------------
DENSE_FIXED = [(("shared", 96, 160, 6), "pattern", 100, range(6)),                       # cached form: one panel and 16 waves per workgroup
               (("shared", 96, 160, 6), "equality", 100, range(6)),
               (("shared", 2112, 2304, 37), "pattern", 50, (0, 15, 16, 31, 32, 36))]     # staged form: two panels per workgroup plus a ragged single panel


@pytest.mark.parametrize("key,kind,K,cols", DENSE_FIXED, ids=[f"{k[1]}x{k[2]}x{k[3]}-{kind}" for k, kind, _, _ in DENSE_FIXED])
def test_dense_fixed_k_iterates_match_the_restatement_per_column(gpu, key, kind, K, cols):
    P, A, Q, L, U = family(*key)
    with gpu.QuadraticProgramSharedBatch(P, A, Q, L, U) as prob:
        prob.set_rho_scale(scale_of(kind, L, U))
        X, flags, infos = prob.solve(numIterations=K, ϵAbs=0.0, ϵRel=0.0, ρ=RHO)
        Z, Y = prob.dual()
    for b in cols:
        ref = reference(key, kind, "reduced", b, numIterations=K, epsAbs=0.0, epsRel=0.0)
        fig = fixed_k_figures(X, Z, Y, infos, b, ref)
        print(f"{key} {kind} column {b}: rel x {fig[0]:.2e} z {fig[1]:.2e} y {fig[2]:.2e} dresPrim {fig[3]:.2e} dresDual {fig[4]:.2e}")
        assert flags[b] == gpu.ConvergenceFlag.convNumItr and infos[b]["iterations"] == K
        assert infos[b]["rhoFinal"] == RHO and infos[b]["rhoProposed"] == RHO          # the base value
        assert fig[0] <= 1e-9 and fig[1] <= 1e-9 and fig[2] <= 1e-8
        assert fig[3] <= 1e-9 and fig[4] <= 1e-9


def test_dense_every_column_stops_at_its_own_iteration(gpu):
    key = ("shared", 96, 160, 6)
    P, A, Q, L, U = family(*key)
    with gpu.QuadraticProgramSharedBatch(P, A, Q, L, U) as prob:
        prob.set_rho_scale(scale_of("equality", L, U))
        X, flags, infos = prob.solve(numIterations=1000, ϵAbs=1e-6, ϵRel=1e-6, ρ=RHO)
    its = []
    for b in range(6):
        ref = reference(key, "equality", "reduced", b, numIterations=1000, epsAbs=1e-6, epsRel=1e-6)
        dev = np.abs(X[b] - ref["x"]).max()
        print(f"column {b}: flag {int(flags[b])}/{ref['convFlag']} iterations {infos[b]['iterations']}/{ref['iterations']} max|x - x_ref| {dev:.2e}")
        assert int(flags[b]) == ref["convFlag"] and infos[b]["iterations"] == ref["iterations"]
        assert dev <= ABS_DEV_THR
        its.append(infos[b]["iterations"])
    assert len(set(its)) > 1, its


def test_dense_columns_and_runs_are_bit_for_bit(gpu):
    key = ("shared", 200, 330, 20)
    P, A, Q, L, U = family(*key)
    s = scale_of("pattern", L, U)
    kw = dict(numIterations=150, ϵAbs=1e-4, ϵRel=1e-4, ρ=RHO)
    with gpu.QuadraticProgramSharedBatch(P, A, Q, L, U) as prob:
        prob.set_rho_scale(s)
        X, flags, infos = prob.solve(**kw)
        Z, Y = prob.dual()
        X2, flags2, infos2 = prob.solve(**kw)
        Z2, Y2 = prob.dual()
    print("iterations:", [i["iterations"] for i in infos])
    assert np.array_equal(X, X2) and np.array_equal(Z, Z2) and np.array_equal(Y, Y2)
    assert [i["iterations"] for i in infos] == [i["iterations"] for i in infos2] and flags == flags2
    for b in (0, 15, 16, 19):
        with gpu.QuadraticProgramSharedBatch(P, A, Q[b:b + 1], L[b:b + 1], U[b:b + 1]) as one:
            one.set_rho_scale(s)
            x1, f1, i1 = one.solve(**kw)
            z1, y1 = one.dual()
        assert f1[0] == flags[b] and i1[0]["iterations"] == infos[b]["iterations"]
        assert np.array_equal(x1[0], X[b]) and np.array_equal(z1[0], Z[b]) and np.array_equal(y1[0], Y[b]), b


def _make(gpu, sparse, P, A, Q, L, U):
    return (gpu.QuadraticProgramSparseSharedBatch if sparse else gpu.QuadraticProgramSharedBatch)(P, A, Q, L, U)


def _run(prob, **kw):
    X, flags, infos = prob.solve(**kw)
    Z, Y = prob.dual()
    return X, Z, Y, [int(f) for f in flags], [i["iterations"] for i in infos]


def _same(a, b):
    return all(np.array_equal(p, q) for p, q in zip(a[:3], b[:3])) and a[3] == b[3] and a[4] == b[4]


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
def test_clearing_restores_the_scalar_path_exactly(gpu, sparse):
    P, A, Q, L, U = family("lasso", 10, 6) if sparse else family("shared", 96, 160, 6)
    kw = dict(numIterations=150, ϵAbs=1e-4, ϵRel=1e-4, ρ=RHO)
    with _make(gpu, sparse, P, A, Q, L, U) as prob:
        first = _run(prob, **kw)
        prob.set_rho_scale(scale_of("pattern", L, U))
        second = _run(prob, **kw)
        prob.set_rho_scale(None)
        third = _run(prob, reuseFactor=True, **kw)
    assert _same(third, first)
    assert not np.array_equal(second[0], first[0]) and not np.array_equal(second[2], first[2])


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
def test_setting_a_scale_invalidates_the_factor(gpu, sparse):
    if sparse:
        P, A, Q, L, U = family("lasso", 10, 6)
        Q2 = Q[::-1].copy()
    else:
        P, A, Q, L, U = family("shared", 96, 160, 6)
        Q2 = shared_family(96, 160, 6, stream=4)[2]
    s = scale_of("equality", L, U)
    kw = dict(numIterations=100, ϵAbs=0.0, ϵRel=0.0, ρ=RHO)
    with _make(gpu, sparse, P, A, Q, L, U) as prob:
        scalar = _run(prob, **kw)
        prob.set_rho_scale(s)
        a = _run(prob, reuseFactor=True, **kw)
        prob.update(mQ=Q2)
        b = _run(prob, reuseFactor=True, **kw)
    with _make(gpu, sparse, P, A, Q, L, U) as fresh:
        fresh.set_rho_scale(s)
        fa = _run(fresh, **kw)
        fresh.update(mQ=Q2)
        fb = _run(fresh, **kw)
    assert _same(a, fa) and _same(b, fb)
    assert not np.array_equal(a[0], scalar[0]) and not np.array_equal(a[0], b[0])


FP32 = [(("shared", 96, 160, 6), "pattern", range(6)), (("shared", 3008, 3072, 17), "equality", (0, 15, 16))]   # cached; staged, a pair with a ragged second panel


@pytest.mark.parametrize("key,kind,cols", FP32, ids=[f"{k[1]}x{k[2]}x{k[3]}-{kind}" for k, kind, _ in FP32])
def test_dense_fp32(gpu, key, kind, cols):
    P, A, Q, L, U = family(*key)
    with gpu.QuadraticProgramSharedBatch(P, A, Q, L, U, dtype="f32") as prob:
        prob.set_rho_scale(scale_of(kind, L, U))
        X, _, infos = prob.solve(numIterations=50, ϵAbs=0.0, ϵRel=0.0, ρ=RHO)
    for b in cols:
        ref = reference(key, kind, "reduced", b, numIterations=50, epsAbs=0.0, epsRel=0.0)
        print(f"fp32 {key} {kind} column {b}: rel x at K = 50 {rel(X[b], ref['x']):.2e}")
        assert infos[b]["iterations"] == 50 and rel(X[b], ref["x"]) <= 1e-3


# ---------------------------------------------------------------------------------------------------------------------
# sparse handle
# ---------------------------------------------------------------------------------------------------------------------
K_SPARSE = 60
SPARSE_FIXED = [(("lasso", 10, 6), "equality", 1e-6, None), (("lasso", 10, 6), "pattern", 1e-6, None),
                (("lasso", 20, 20), "equality", 1e-6, None), (("lasso", 20, 20), "pattern", 1e-6, None),
                (("random", 20), "pattern", 1e-9, None),          # all tail: every constraint row sits in the dense tail
                (("random", 20), "pattern", 1e-9, "64")]          # QPS_LDL_MAX_TAIL = 64: constraint rows in the sparse levels as well as in the tail


@pytest.mark.parametrize("key,kind,tol,max_tail", SPARSE_FIXED, ids=[f"{k[0]}{'x'.join(map(str, k[1:]))}-{kind}-tail{t}" for k, kind, _, t in SPARSE_FIXED])
def test_sparse_fixed_k_iterates_match_the_restatement_per_column(gpu, monkeypatch, key, kind, tol, max_tail):
    P, A, Q, L, U = family(*key)
    if max_tail:
        monkeypatch.setenv("QPS_LDL_MAX_TAIL", max_tail)
    else:
        monkeypatch.delenv("QPS_LDL_MAX_TAIL", raising=False)
    with gpu.QuadraticProgramSparseSharedBatch(P, A, Q, L, U) as prob:
        prob.set_rho_scale(scale_of(kind, L, U))
        X, flags, infos = prob.solve(numIterations=K_SPARSE, ϵAbs=0.0, ϵRel=0.0, ρ=RHO)
        Z, Y = prob.dual()
    for b in range(Q.shape[0]):
        ref = reference(key, kind, "kkt", b, numIterations=K_SPARSE, epsAbs=0.0, epsRel=0.0)
        fig = fixed_k_figures(X, Z, Y, infos, b, ref)
        print(f"{key} {kind} tail {max_tail} column {b}: rel x {fig[0]:.2e} z {fig[1]:.2e} y {fig[2]:.2e} dresPrim {fig[3]:.2e} dresDual {fig[4]:.2e}")
        assert flags[b] == gpu.ConvergenceFlag.convNumItr and infos[b]["iterations"] == K_SPARSE
        assert infos[b]["rhoFinal"] == RHO and infos[b]["rhoProposed"] == RHO
        assert fig[0] <= tol and fig[1] <= tol and fig[2] <= 10 * tol, (key, b, fig)
        assert fig[3] <= tol and fig[4] <= 10 * tol, (key, b, fig)


def test_sparse_columns_are_bit_for_bit(gpu):
    P, A, Q, L, U = family("lasso", 20, 20)
    s = scale_of("pattern", L, U)
    kw = dict(numIterations=K_SPARSE, ϵAbs=0.0, ϵRel=0.0, ρ=RHO)
    with gpu.QuadraticProgramSparseSharedBatch(P, A, Q, L, U) as prob:
        prob.set_rho_scale(s)
        full = _run(prob, **kw)
    for b in (0, 16, 19):
        with gpu.QuadraticProgramSparseSharedBatch(P, A, Q[b:b + 1], L[b:b + 1], U[b:b + 1]) as one:
            one.set_rho_scale(s)
            x1, z1, y1, _, _ = _run(one, **kw)
        assert np.array_equal(x1[0], full[0][b]) and np.array_equal(z1[0], full[1][b]) and np.array_equal(y1[0], full[2][b]), b


def test_sparse_fp32(gpu):
    key = ("random", 4)
    P, A, Q, L, U = family(*key)
    with gpu.QuadraticProgramSparseSharedBatch(P, A, Q, L, U, dtype="f32") as prob:
        prob.set_rho_scale(scale_of("pattern", L, U))
        X, _, _ = prob.solve(numIterations=50, ϵAbs=0.0, ϵRel=0.0, ρ=RHO)
    for b in range(4):
        ref = reference(key, "pattern", "kkt", b, numIterations=50, epsAbs=0.0, epsRel=0.0)
        print(f"sparse fp32 column {b}: rel x {rel(X[b], ref['x']):.2e}")
        assert rel(X[b], ref["x"]) <= 1e-3


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
def test_bad_scales_are_refused_and_the_handle_keeps_its_state(gpu, sparse):
    P, A, Q, L, U = family("random", 4) if sparse else family("shared", 96, 160, 6)
    m = A.shape[0]
    kw = dict(numIterations=100, ϵAbs=0.0, ϵRel=0.0, ρ=RHO)
    good = scale_of("pattern", L, U)
    with _make(gpu, sparse, P, A, Q, L, U) as prob:
        plain = _run(prob, **kw)
        for pos, bad in ((0, 0.0), (m // 2, -1.0), (m - 1, np.nan), (3, np.inf), (5, -np.inf)):
            s = good.copy(); s[pos] = bad
            with pytest.raises(gpu.QpsError) as e:
                prob.set_rho_scale(s)
            assert e.value.status == BAD_ARGUMENT and str(pos) in e.value.message, (bad, e.value.message)
            assert _same(_run(prob, reuseFactor=True, **kw), plain), bad
        with pytest.raises(ValueError):
            prob.set_rho_scale(good[:-1])
        prob.set_rho_scale(good)
        scaled = _run(prob, **kw)
        s = good.copy(); s[1] = 0.0
        with pytest.raises(gpu.QpsError):
            prob.set_rho_scale(s)
        assert _same(_run(prob, reuseFactor=True, **kw), scaled)          # the previous scale and its factor stay
        with pytest.raises(gpu.QpsError) as e:
            prob.solve(adptΡ=True, **kw)
        assert e.value.status == UNSUPPORTED and "adptRho" in e.value.message
        assert _same(_run(prob, reuseFactor=True, **kw), scaled)
    assert not np.array_equal(scaled[0], plain[0])


def test_other_handles_are_unsupported(gpu):
    from quadraticprogramsolver_amd import _lib
    P, A, Q, L, U = family("shared", 96, 160, 6)
    s = np.ones(A.shape[0])
    ptr = s.ctypes.data_as(C.POINTER(C.c_double))
    with gpu.QuadraticProgram(P, Q[0], A, L[0], U[0]) as one:
        assert _lib.lib().qps_set_shared_rho_scale(one._h, ptr) == UNSUPPORTED
        assert b"shared-matrix batch" in _lib.lib().qps_last_error(one._h)
        assert _lib.lib().qps_set_shared_rho_scale(one._h, None) == UNSUPPORTED
    with gpu.QuadraticProgramBatch([(P, Q[b], A, L[b], U[b]) for b in range(2)]) as batch:
        assert _lib.lib().qps_set_shared_rho_scale(batch._h, ptr) == UNSUPPORTED
        assert b"shared-matrix batch" in _lib.lib().qps_last_error(batch._h)
