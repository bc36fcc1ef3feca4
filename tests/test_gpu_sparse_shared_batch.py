"""Sparse shared-matrix batch on the device (qps_create_csc_shared_batch): every column of a family that shares a sparse mP and mA behaves as a
stand-alone solve of the C oracle's sparse L D L' plugin on (P, q_b, A, l_b, u_b) with a fixed rho.

Tolerances are those of tests/test_gpu_ldl.py: 1e-9 relative on x and z and 1e-8 on y where K is well conditioned (randomQp); 1e-6 / 1e-5 for the
lasso class, whose K carries pivots of size sigma (two correct factorisations with different orderings differ by ~1e-16 cond(K)); residuals as in
test_ldl_iterates_match_oracle_all_classes."""
import functools

import numpy as np
import pytest

from sparse_shared_cases import RANDOM_FAMILY_ORACLE_ITERATIONS, lasso_path, random_family
from test_gpu_parity import rel

pytestmark = pytest.mark.gpu

UNSUPPORTED = 8
K_FIXED = 60


@functools.lru_cache(maxsize=None)
def family(name, size, count):
    return lasso_path(size, count) if name == "lasso" else random_family(count)


_ORACLE = {}


def oracle(c_oracle, key, b, **kw):
    """One C-oracle solve per (family, column, parameters), shared by the tests of this module."""
    k = (key, b, tuple(sorted(kw.items())))
    if k not in _ORACLE:
        P, A, Q, L, U = family(*key)
        _ORACLE[k] = c_oracle.solve(P, Q[b], A, L[b], U[b], rho=0.1, linsys=c_oracle.KIND_KKT_LDL_SPARSE, **kw)
    return _ORACLE[k]


def check_fixed_k(c_oracle, key, X, Z, Y, flags, infos, gpu, tol, tag=""):
    count = X.shape[0]
    worst = np.zeros(5)
    for b in range(count):
        xo, io = oracle(c_oracle, key, b, numIterations=K_FIXED, epsAbs=0.0, epsRel=0.0)
        fig = (rel(X[b], xo), rel(Z[b], io["z"]), rel(Y[b], io["y"]), abs(infos[b]["resPrim"] - io["resPrim"]) / max(1.0, io["resPrim"]),
               abs(infos[b]["resDual"] - io["resDual"]) / max(1.0, io["resDual"]))
        worst = np.maximum(worst, fig)
        print(f"{key}{tag} column {b}: rel x {fig[0]:.2e} z {fig[1]:.2e} y {fig[2]:.2e} dresPrim {fig[3]:.2e} dresDual {fig[4]:.2e}")
        assert flags[b] == gpu.ConvergenceFlag.convNumItr and infos[b]["iterations"] == K_FIXED
        assert fig[0] <= tol and fig[1] <= tol and fig[2] <= 10 * tol, (key, b, fig)
        assert fig[3] <= tol and fig[4] <= 10 * tol, (key, b, fig)
        assert infos[b]["sweepVariant"] == 0 and infos[b]["trsvBlock"] == 0 and infos[b]["numRefactor"] == 0
    return worst


FIXED_CASES = [(("lasso", 10, 6), 1e-6), (("lasso", 20, 20), 1e-6), (("random", 100, 20), 1e-9)]


@pytest.mark.parametrize("key,tol", FIXED_CASES, ids=[f"{k[0]}{k[1]}x{k[2]}" for k, _ in FIXED_CASES])
def test_fixed_k_iterates_match_the_oracle_per_column(gpu, c_oracle, key, tol):
    """eps 0, K = 60, rho = 0.1, fp64.  lasso: sparse levels plus a tail (20 columns: two panels, a ragged second one); random_family: tail only."""
    P, A, Q, L, U = family(*key)
    with gpu.QuadraticProgramSparseSharedBatch(P, A, Q, L, U) as prob:
        X, flags, infos = prob.solve(numIterations=K_FIXED, ϵAbs=0.0, ϵRel=0.0, ρ=0.1)
        Z, Y = prob.dual()
    assert X.shape == Q.shape and Z.shape == L.shape and Y.shape == L.shape
    check_fixed_k(c_oracle, key, X, Z, Y, flags, infos, gpu, tol)


@pytest.mark.parametrize("spr", [None, "1", "4", "16"])
def test_every_strip_count(gpu, c_oracle, monkeypatch, spr):
    """QPS_LDL_MAX_TAIL = 64 turns randomQp 100 into 86 sparse columns in 37 levels of long rows plus a 64-row tail; QPS_LDL_PANEL_SPR forces each
    instantiation of the sweep kernels over all of them."""
    key = ("random", 100, 20)
    P, A, Q, L, U = family(*key)
    monkeypatch.setenv("QPS_LDL_MAX_TAIL", "64")
    if spr is None:
        monkeypatch.delenv("QPS_LDL_PANEL_SPR", raising=False)
    else:
        monkeypatch.setenv("QPS_LDL_PANEL_SPR", spr)
    with gpu.QuadraticProgramSparseSharedBatch(P, A, Q, L, U) as prob:
        X, flags, infos = prob.solve(numIterations=K_FIXED, ϵAbs=0.0, ϵRel=0.0, ρ=0.1)
        Z, Y = prob.dual()
    check_fixed_k(c_oracle, key, X, Z, Y, flags, infos, gpu, 1e-9, tag=f" spr={spr}")


def test_every_column_stops_at_its_own_iteration(gpu, c_oracle):
    key = ("random", 100, 20)
    P, A, Q, L, U = family(*key)
    with gpu.QuadraticProgramSparseSharedBatch(P, A, Q, L, U) as prob:
        X, flags, infos = prob.solve(ϵAbs=1e-6, ϵRel=1e-6, ρ=0.1)
    its = []
    for b in range(20):
        xo, io = oracle(c_oracle, key, b, numIterations=5000, epsAbs=1e-6, epsRel=1e-6)
        dev = np.abs(X[b] - xo).max()
        print(f"column {b}: flag {int(flags[b])}/{io['convFlag']} iterations {infos[b]['iterations']}/{io['iterations']} max|x - x_oracle| {dev:.2e}")
        assert int(flags[b]) == io["convFlag"] and infos[b]["iterations"] == io["iterations"]
        assert dev <= 1e-5
        its.append(infos[b]["iterations"])
    assert its == RANDOM_FAMILY_ORACLE_ITERATIONS and len(set(its)) > 1, its


def test_columns_are_independent_and_runs_repeat_bit_for_bit(gpu):
    """The summation order of an element depends on the factor's pattern and the strip count only: column b of a count-20 solve equals, bit for bit,
    the same data in a count-1 handle; two solves of one handle are bit-identical."""
    P, A, Q, L, U = family("lasso", 10, 20)
    kw = dict(numIterations=150, ϵAbs=1e-4, ϵRel=1e-4, ρ=0.1)
    with gpu.QuadraticProgramSparseSharedBatch(P, A, Q, L, U) as prob:
        X, flags, infos = prob.solve(**kw)
        Z, Y = prob.dual()
        X2, flags2, infos2 = prob.solve(**kw)
        Z2, Y2 = prob.dual()
    print("iterations:", [i["iterations"] for i in infos])
    assert np.array_equal(X, X2) and np.array_equal(Z, Z2) and np.array_equal(Y, Y2)
    assert [i["iterations"] for i in infos] == [i["iterations"] for i in infos2]
    for b in (0, 1, 15, 16, 19):                                 # both panels, first and last column of each
        with gpu.QuadraticProgramSparseSharedBatch(P, A, Q[b:b + 1], L[b:b + 1], U[b:b + 1]) as one:
            x1, f1, i1 = one.solve(**kw)
            z1, y1 = one.dual()
        assert f1[0] == flags[b] and i1[0]["iterations"] == infos[b]["iterations"]
        assert np.array_equal(x1[0], X[b]) and np.array_equal(z1[0], Z[b]) and np.array_equal(y1[0], Y[b]), b
    # the same with columns that stop at different checks and are frozen while their neighbours go on (random_family: 200, 75, ..., 50 iterations)
    P, A, Q, L, U = family("random", 100, 20)
    kw = dict(ϵAbs=1e-6, ϵRel=1e-6, ρ=0.1)
    with gpu.QuadraticProgramSparseSharedBatch(P, A, Q, L, U) as prob:
        X, flags, infos = prob.solve(**kw)
        Z, Y = prob.dual()
    assert len({i["iterations"] for i in infos}) > 1
    for b in (0, 1, 19):
        with gpu.QuadraticProgramSparseSharedBatch(P, A, Q[b:b + 1], L[b:b + 1], U[b:b + 1]) as one:
            x1, f1, i1 = one.solve(**kw)
            z1, y1 = one.dual()
        assert f1[0] == flags[b] and i1[0]["iterations"] == infos[b]["iterations"]
        assert np.array_equal(x1[0], X[b]) and np.array_equal(z1[0], Z[b]) and np.array_equal(y1[0], Y[b]), b


def test_columns_match_the_stand_alone_handle(gpu, c_oracle):
    """Columns 0 and 19 of the lasso 20 family against QuadraticProgram(..., linsys="ldl") at the same K: both within the oracle tolerance of the
    oracle (and so of each other), same flag."""
    key = ("lasso", 20, 20)
    P, A, Q, L, U = family(*key)
    with gpu.QuadraticProgramSparseSharedBatch(P, A, Q, L, U) as prob:
        X, flags, infos = prob.solve(numIterations=K_FIXED, ϵAbs=0.0, ϵRel=0.0, ρ=0.1)
        Z, Y = prob.dual()
    for b in (0, 19):
        x = np.zeros(P.shape[0]); info = {}
        with gpu.QuadraticProgram(P, Q[b], A, L[b], U[b], linsys="ldl") as one:
            flag = one.solve(x, numIterations=K_FIXED, ϵAbs=0.0, ϵRel=0.0, ρ=0.1, info=info)
            z, y = one.dual()
        xo, io = oracle(c_oracle, key, b, numIterations=K_FIXED, epsAbs=0.0, epsRel=0.0)
        fig = (rel(X[b], x), rel(Z[b], z), rel(Y[b], y), rel(x, xo))
        print(f"column {b}: batch vs stand-alone rel x {fig[0]:.2e} z {fig[1]:.2e} y {fig[2]:.2e}; stand-alone vs oracle rel x {fig[3]:.2e}")
        assert flag == flags[b] and info["iterations"] == infos[b]["iterations"]
        assert fig[0] <= 1e-6 and fig[1] <= 1e-6 and fig[2] <= 1e-5


def test_vector_update_keeps_the_factor(gpu):
    """update() then solve(reuseFactor=True) equals a freshly created handle on the new vectors bit for bit (also after a partial update), and the reused
    solve's tSetup -- warm starts up, state cleared -- is below the first solve's, which ran the numeric factorisation."""
    P, A, Q, L, U = family("lasso", 20, 20)
    Q2, L2, U2 = Q[::-1].copy(), L - 0.5, U + 0.25
    kw = dict(numIterations=50, ϵAbs=0.0, ϵRel=0.0, ρ=0.1)
    with gpu.QuadraticProgramSparseSharedBatch(P, A, Q, L, U) as prob:
        _, _, i0 = prob.solve(**kw)
        prob.update(Q2, L2, U2)
        Xa, _, ia = prob.solve(reuseFactor=True, **kw)
        Za, Ya = prob.dual()
        prob.update(mQ=Q)
        Xc, _, _ = prob.solve(reuseFactor=True, **kw)
        Zc, Yc = prob.dual()
    with gpu.QuadraticProgramSparseSharedBatch(P, A, Q2, L2, U2) as fresh:
        Xb, _, _ = fresh.solve(**kw)
        Zb, Yb = fresh.dual()
    with gpu.QuadraticProgramSparseSharedBatch(P, A, Q, L2, U2) as fresh:
        Xd, _, _ = fresh.solve(**kw)
        Zd, Yd = fresh.dual()
    print(f"tSetup first solve {i0[0]['tSetup'] * 1e3:.3f} ms (numeric factorisation), reused {ia[0]['tSetup'] * 1e3:.3f} ms")
    assert np.array_equal(Xa, Xb) and np.array_equal(Za, Zb) and np.array_equal(Ya, Yb)
    assert np.array_equal(Xc, Xd) and np.array_equal(Zc, Zd) and np.array_equal(Yc, Yd)
    assert not np.array_equal(Xa, Xc)
    assert ia[0]["tSetup"] < i0[0]["tSetup"]


@pytest.mark.parametrize("max_tail", [None, "64"])
def test_fp32(gpu, c_oracle, monkeypatch, max_tail):
    """fp32 panels against the fp64 oracle, the bound of test_fp32_path; all tail, and sparse levels plus a tail."""
    key = ("random", 100, 4)
    P, A, Q, L, U = family(*key)
    if max_tail:
        monkeypatch.setenv("QPS_LDL_MAX_TAIL", max_tail)
    with gpu.QuadraticProgramSparseSharedBatch(P, A, Q, L, U, dtype="f32") as prob:
        X, flags, infos = prob.solve(numIterations=50, ϵAbs=0.0, ϵRel=0.0, ρ=0.1)
    for b in range(4):
        xo, _ = oracle(c_oracle, key, b, numIterations=50, epsAbs=0.0, epsRel=0.0)
        print(f"fp32 max_tail={max_tail} column {b}: rel x {rel(X[b], xo):.2e}")
        assert rel(X[b], xo) <= 1e-3


def test_refusals_leave_the_handle_usable(gpu, c_oracle):
    key = ("random", 100, 20)
    P, A, Q, L, U = family(*key)
    with gpu.QuadraticProgramSparseSharedBatch(P, A, Q, L, U) as prob:
        for kw, word in ((dict(adptΡ=True), "adptRho"), (dict(polish=True), "polish"), (dict(linsys="cg"), "linsys")):
            with pytest.raises(gpu.QpsError) as e:
                prob.solve(numIterations=K_FIXED, ρ=0.1, **kw)
            assert e.value.status == UNSUPPORTED and word in str(e.value), (kw, str(e.value))
        X, flags, infos = prob.solve(numIterations=K_FIXED, ϵAbs=0.0, ϵRel=0.0, ρ=0.1, linsys="ldl", trsvBlock=7)
        Z, Y = prob.dual()
    check_fixed_k(c_oracle, key, X, Z, Y, flags, infos, gpu, 1e-9)


def test_lifecycle_and_profile_categories(gpu):
    """Create, solve and destroy twice in one process; a profiled solve reports the categories of the panel loop."""
    P, A, Q, L, U = family("lasso", 10, 6)
    first = None
    for _ in range(2):
        prob = gpu.QuadraticProgramSparseSharedBatch(P, A, Q, L, U)
        prob.set_profiling(2)
        X, _, _ = prob.solve(numIterations=50, ϵAbs=0.0, ϵRel=0.0, ρ=0.1)
        kt = {k["name"]: k for k in prob.kernel_times()}
        prob.close()
        for word in ("rhs", "forward levels", "tail", "backward levels", "post + update", "check"):
            hit = [k for name, k in kt.items() if name.startswith("sparse shared:") and word in name]
            assert len(hit) == 1 and hit[0]["launches"] > 0 and hit[0]["algo_bytes"] > 0, (word, sorted(kt))
        assert first is None or np.array_equal(first, X)
        first = X
