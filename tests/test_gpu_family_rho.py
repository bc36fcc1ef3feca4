"""Family-wide adaptive rho of the shared-matrix batches on the device (qps_set_shared_adaptive_rho, mode 1): ONE rho moves for all columns by the reference's
rule with the norms of the worst running columns, and every column behaves as the numpy restatement of tests/family_rho_cases.py -- its reduced Cholesky form
for the dense handle, its dense KKT form for the sparse one.  Base rho = 0.1, eps = 1e-6, numItrConv = 25; the cases and their CPU figures are the table there,
and tests/test_family_rho_cpu.py keeps every decision of every case at least 2 % away from a rounding edge.

Bounds are those of tests/test_gpu_rho_scale.py for the same families: dense fp64 and sparse random 1e-9 relative on x and z, 1e-8 on y; lasso 1e-6 / 1e-5; fp32
1e-3.  rhoFinal: 1e-12 relative at count = 1 against the C oracle, 1e-10 on the dense cases.  On the sparse cases the two exact forms of the restatement
disagree among themselves in the switched rho -- a late proposal divides residual norms that have shrunk by orders of magnitude: 1.5e-9 on lasso10-f4 (fourth
switch), 5.9e-6 on lasso10-eq-f4 (fourth switch, rho_i up to 1e5), 2.8e-9 on random20-f5 (second switch), 2.5e-14 on the fixed-K pattern case.  The case
table records that disagreement (``rho_spread``, held by the CPU guard), and the device -- a third implementation, with its own summation orders -- is held to
ten times it, and to no less than the dense bound of 1e-10."""
import functools

import numpy as np
import pytest

from family_rho_cases import CASES, EPS, NUM_ITR_CONV, RHO, case_data, case_run
from test_gpu_parity import rel

pytestmark = pytest.mark.gpu

BAD_ARGUMENT, UNSUPPORTED = 1, 8
KW = dict(ϵAbs=EPS, ϵRel=EPS, ρ=RHO, numItrConv=NUM_ITR_CONV)


@functools.lru_cache(maxsize=None)
def data(name):
    return case_data(name)


def _make(gpu, sparse, P, A, Q, L, U, **kw):
    return (gpu.QuadraticProgramSparseSharedBatch if sparse else gpu.QuadraticProgramSharedBatch)(P, A, Q, L, U, **kw)


def _run(prob, **kw):
    X, flags, infos = prob.solve(**kw)
    Z, Y = prob.dual()
    return X, Z, Y, [int(f) for f in flags], infos


def _same(a, b):
    keys = ("iterations", "numRefactor", "rhoFinal", "rhoProposed", "resPrim", "resDual")
    return all(np.array_equal(p, q) for p, q in zip(a[:3], b[:3])) and a[3] == b[3] and [[i[k] for k in keys] for i in a[4]] == [[i[k] for k in keys] for i in b[4]]


def compare_with_restatement(name, run, ref, xz_tol, y_tol, rho_tol):
    X, Z, Y, flags, infos = run
    for b, col in enumerate(ref["columns"]):
        fig = (rel(X[b], col["x"]), rel(Z[b], col["z"]), rel(Y[b], col["y"]), abs(infos[b]["rhoFinal"] - col["rhoFinal"]) / col["rhoFinal"])
        print(f"{name} column {b}: flag {flags[b]}/{col['convFlag']} iterations {infos[b]['iterations']}/{col['iterations']} numRefactor "
              f"{infos[b]['numRefactor']}/{col['numRefactor']} rhoFinal {infos[b]['rhoFinal']:.12g} (rel {fig[3]:.2e}) rel x {fig[0]:.2e} z {fig[1]:.2e} y {fig[2]:.2e}")
    for b, col in enumerate(ref["columns"]):
        fig = (rel(X[b], col["x"]), rel(Z[b], col["z"]), rel(Y[b], col["y"]), abs(infos[b]["rhoFinal"] - col["rhoFinal"]) / col["rhoFinal"])
        assert flags[b] == col["convFlag"] and infos[b]["iterations"] == col["iterations"] and infos[b]["numRefactor"] == col["numRefactor"], (name, b)
        assert fig[3] <= rho_tol, (name, b, fig)
        # The proposal after a column's last check divides residual norms that have come down to eps = 1e-6 of their vectors: iterates that are held to xz_tol
        # give those norms, and the proposal, to xz_tol / eps only -- 1e-3 where the iterates are held to 1e-9.  On lasso (iterates held to 1e-6) that says
        # nothing; there the proposal is the same kind of quantity as the switched rho and is held to the case's rhoFinal bound, but to no less than 1e-6.
        # A wrong choice of the two columns, or a proposal booked to the wrong column, changes it in the first digits.
        dprop = abs(infos[b]["rhoProposed"] - col["rhoProposed"]) / col["rhoProposed"]
        print(f"{name} column {b}: rhoProposed {infos[b]['rhoProposed']:.9g} against {col['rhoProposed']:.9g} (rel {dprop:.2e})")
        assert dprop <= (xz_tol / EPS if xz_tol / EPS < 1.0 else max(rho_tol, 1e-6)), (name, b, infos[b]["rhoProposed"], col["rhoProposed"])
        assert fig[0] <= xz_tol and fig[1] <= xz_tol and fig[2] <= y_tol, (name, b, fig)
        assert infos[b]["tRefactor"] > 0 and infos[b]["tRefactor"] < infos[b]["tLoop"]


# ---------------------------------------------------------------------------------------------------------------------
# 1. count = 1: the reference's adptRho loop
# ---------------------------------------------------------------------------------------------------------------------
def test_count_one_is_the_adaptive_loop_of_the_oracle(gpu, c_oracle):
    """Column 0 of shared_family(96, 160, 4) alone on a dense shared handle under mode 1 against the C oracle with adptRho = 1: same flag, iterations and
    numRefactor, rhoFinal to 1e-12 relative, x and z within 1e-9, y within 1e-8."""
    P, A, Q, L, U, _, _ = data("shared96-f5")
    xo, io = c_oracle.solve(P, Q[0], A, L[0], U[0], rho=RHO, adptRho=True, fctrRho=5.0, numIterations=5000, epsAbs=EPS, epsRel=EPS, numItrConv=NUM_ITR_CONV)
    with gpu.QuadraticProgramSharedBatch(P, A, Q[:1], L[:1], U[:1]) as prob:
        prob.set_adaptive_rho()
        X, Z, Y, flags, infos = _run(prob, fctrΡ=5, **KW)
    i = infos[0]
    fig = (rel(X[0], xo), rel(Z[0], io["z"]), rel(Y[0], io["y"]), abs(i["rhoFinal"] - io["rhoFinal"]) / io["rhoFinal"])
    print(f"count 1: flag {flags[0]}/{io['convFlag']} iterations {i['iterations']}/{io['iterations']} numRefactor {i['numRefactor']}/{io['numRefactor']} "
          f"rhoFinal {i['rhoFinal']!r}/{io['rhoFinal']!r} (rel {fig[3]:.2e}) rel x {fig[0]:.2e} z {fig[1]:.2e} y {fig[2]:.2e}")
    assert flags[0] == io["convFlag"] and i["iterations"] == io["iterations"] and i["numRefactor"] == io["numRefactor"] >= 1
    assert fig[3] <= 1e-12
    assert fig[0] <= 1e-9 and fig[1] <= 1e-9 and fig[2] <= 1e-8


# ---------------------------------------------------------------------------------------------------------------------
# 2. dense handle, every column against the restatement
# ---------------------------------------------------------------------------------------------------------------------
# the last one: the STAGED kernel form (matrices above the 32 MiB cut; 37 columns = two panels per workgroup and a ragged single one) to eps = 1e-6 with
# numIterations = 175: after the switch at iteration 26, fifteen columns of the first panel take their own flag and stopping iteration (75 .. 175) and are frozen
# while the others go on to iteration 175 and end with flag 1 (why not further: tests/family_rho_cases.py)
DENSE = ["shared96-f5", "shared96-f3", "shared96-eq-f5", "shared200-f5", "shared200-eq-f5", "shared2112-f5-n175"]


@pytest.mark.parametrize("name", DENSE)
def test_dense_columns_match_the_restatement(gpu, name):
    P, A, Q, L, U, s, f = data(name)
    with gpu.QuadraticProgramSharedBatch(P, A, Q, L, U) as prob:
        if s is not None:
            prob.set_rho_scale(s)
        prob.set_adaptive_rho()
        run = _run(prob, fctrΡ=f, numIterations=CASES[name].get("num_iterations", 5000), **KW)
    compare_with_restatement(name, run, case_run(name, "reduced"), 1e-9, 1e-8, 1e-10)
    assert [i["iterations"] for i in run[4]] == CASES[name]["iterations"]


def test_dense_staged_kernels_switch_and_match_the_restatement(gpu):
    """Matrices above the 32 MiB cut run the staged kernel form, two panels per workgroup and a ragged single one (the shapes of tests/test_gpu_shared_batch.py);
    with the equality scale (factor 10), fixed K = 60 with the switch of the case table in it: the scaled form of the w kernel reads the row rho that the switch
    pushed.  The listed columns against the restatement of the whole batch.  (Without a scale the staged form runs to eps in
    test_dense_columns_match_the_restatement.)"""
    name = "shared2112-eq10-f5-k60"
    P, A, Q, L, U, scale, f = data(name)
    K = CASES[name]["fixed_k"]
    ref = case_run(name, "reduced")
    with gpu.QuadraticProgramSharedBatch(P, A, Q, L, U) as prob:
        prob.set_rho_scale(scale)
        prob.set_adaptive_rho()
        X, Z, Y, flags, infos = _run(prob, numIterations=K, ϵAbs=0.0, ϵRel=0.0, ρ=RHO, fctrΡ=f)
    assert [s[0] for s in ref["switches"]] == CASES[name]["switches"]
    for b in (0, 15, 16, 31, 32, 36):
        col = ref["columns"][b]
        fig = (rel(X[b], col["x"]), rel(Z[b], col["z"]), rel(Y[b], col["y"]), abs(infos[b]["rhoFinal"] - col["rhoFinal"]) / col["rhoFinal"])
        print(f"staged column {b}: numRefactor {infos[b]['numRefactor']}/{col['numRefactor']} rhoFinal {infos[b]['rhoFinal']:.12g} (rel {fig[3]:.2e}) "
              f"rel x {fig[0]:.2e} z {fig[1]:.2e} y {fig[2]:.2e}")
        assert flags[b] == 1 and infos[b]["iterations"] == K and infos[b]["numRefactor"] == col["numRefactor"] == len(CASES[name]["switches"])
        assert fig[3] <= 1e-10
        assert fig[0] <= 1e-9 and fig[1] <= 1e-9 and fig[2] <= 1e-8


# ---------------------------------------------------------------------------------------------------------------------
# 3. sparse handle
# ---------------------------------------------------------------------------------------------------------------------
SPARSE = [("lasso10-f4", None, 1e-6, 1e-5), ("lasso10-eq-f4", None, 1e-6, 1e-5),                 # sparse levels and a dense tail
          ("random20-f5", None, 1e-9, 1e-8),        # all tail: every constraint row sits in the dense tail
          ("random20-f5", "64", 1e-9, 1e-8),        # QPS_LDL_MAX_TAIL = 64: constraint rows in the sparse levels as well as in the tail
          ("random20-pat-f5-k175", "64", 1e-9, 1e-8)]   # pattern_rho_scale, fixed K


@pytest.mark.parametrize("name,max_tail,xz_tol,y_tol", SPARSE, ids=[f"{n}-tail{t}" for n, t, _, _ in SPARSE])
def test_sparse_columns_match_the_restatement(gpu, monkeypatch, name, max_tail, xz_tol, y_tol):
    P, A, Q, L, U, s, f = data(name)
    rho_tol = max(1e-10, 10.0 * CASES[name].get("rho_spread", 1e-11))          # (module docstring)
    if max_tail:
        monkeypatch.setenv("QPS_LDL_MAX_TAIL", max_tail)
    else:
        monkeypatch.delenv("QPS_LDL_MAX_TAIL", raising=False)
    with gpu.QuadraticProgramSparseSharedBatch(P, A, Q, L, U) as prob:
        if s is not None:
            prob.set_rho_scale(s)
        prob.set_adaptive_rho()
        K = CASES[name].get("fixed_k")
        run = _run(prob, fctrΡ=f, **(dict(numIterations=K, ϵAbs=0.0, ϵRel=0.0, ρ=RHO, numItrConv=NUM_ITR_CONV) if K else KW))
    compare_with_restatement(f"{name} tail {max_tail}", run, case_run(name, "kkt"), xz_tol, y_tol, rho_tol)
    assert [i["iterations"] for i in run[4]] == CASES[name]["iterations"]


# ---------------------------------------------------------------------------------------------------------------------
# 4. what the rule is for: the lasso path at rho = 0.1
# ---------------------------------------------------------------------------------------------------------------------
def test_lasso_path_converges_only_under_the_family_rule(gpu):
    name = "lasso10-f4"
    P, A, Q, L, U, _, f = data(name)
    with gpu.QuadraticProgramSparseSharedBatch(P, A, Q, L, U) as prob:
        _, flags0, infos0 = prob.solve(fctrΡ=f, **KW)
        prob.set_adaptive_rho()
        _, flags1, infos1 = prob.solve(fctrΡ=f, **KW)
    print("fixed rho:", [(int(fl), i["iterations"]) for fl, i in zip(flags0, infos0)], " family rule:", [(int(fl), i["iterations"]) for fl, i in zip(flags1, infos1)])
    assert [int(fl) for fl in flags0] == [1] * 6 and [i["iterations"] for i in infos0] == [5000] * 6
    assert all(i["numRefactor"] == 0 and i["rhoFinal"] == RHO and i["tRefactor"] == 0 for i in infos0)
    assert all(int(fl) in (2, 3) for fl in flags1)
    assert [int(fl) for fl in flags1] == CASES[name]["flags"] and [i["iterations"] for i in infos1] == CASES[name]["iterations"]


# ---------------------------------------------------------------------------------------------------------------------
# 5. fp32
# ---------------------------------------------------------------------------------------------------------------------
def test_dense_fp32_switches_where_fp64_does(gpu):
    """The fctrRho = 5 case at a fixed K (eps = 0), as the fp32 cases of tests/test_gpu_rho_scale.py: the restatement switches at the top of iteration 26 and nowhere
    else up to K = 100, so numRefactor is 0 after 25 iterations and 1 after 26 and after 100; x, z, y within 1e-3 relative."""
    name = "shared96-f5-k100"
    P, A, Q, L, U, _, f = data(name)
    ref = case_run(name, "reduced")
    assert [s[0] for s in ref["switches"]] == [26]
    with gpu.QuadraticProgramSharedBatch(P, A, Q, L, U, dtype="f32") as prob:
        prob.set_adaptive_rho()
        for K, want in ((25, 0), (26, 1)):
            _, _, infos = prob.solve(numIterations=K, ϵAbs=0.0, ϵRel=0.0, ρ=RHO, fctrΡ=f)
            assert [i["numRefactor"] for i in infos] == [want] * 4 and [i["iterations"] for i in infos] == [K] * 4, (K, infos)
        X, Z, Y, flags, infos = _run(prob, numIterations=100, ϵAbs=0.0, ϵRel=0.0, ρ=RHO, fctrΡ=f)
    for b, col in enumerate(ref["columns"]):
        fig = (rel(X[b], col["x"]), rel(Z[b], col["z"]), rel(Y[b], col["y"]), abs(infos[b]["rhoFinal"] - col["rhoFinal"]) / col["rhoFinal"])
        print(f"fp32 column {b}: numRefactor {infos[b]['numRefactor']} rhoFinal {infos[b]['rhoFinal']:.8g} (rel {fig[3]:.2e}) rel x {fig[0]:.2e} z {fig[1]:.2e} y {fig[2]:.2e}")
        assert infos[b]["numRefactor"] == 1 and infos[b]["iterations"] == 100
        assert max(fig) <= 1e-3


# ---------------------------------------------------------------------------------------------------------------------
# 6. invariants and refusals
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
def test_mode_zero_is_the_untouched_path_and_runs_repeat(gpu, sparse):
    name = "lasso10-f4" if sparse else "shared96-eq-f5"
    P, A, Q, L, U, s, f = data(name)
    fixed = dict(numIterations=300, fctrΡ=f, **KW)
    with _make(gpu, sparse, P, A, Q, L, U) as never:
        if s is not None:
            never.set_rho_scale(s)
        plain = _run(never, **fixed)
    with _make(gpu, sparse, P, A, Q, L, U) as prob:
        if s is not None:
            prob.set_rho_scale(s)
        prob.set_adaptive_rho(False)
        zero = _run(prob, **fixed)
        prob.set_adaptive_rho()
        one = _run(prob, **fixed)
        again = _run(prob, **fixed)                      # the mode stays with the handle; the factor of the last rho is replaced by the one of rho = 0.1
        prob.set_adaptive_rho(False)
        back = _run(prob, **fixed)
    assert _same(zero, plain) and _same(back, plain)
    assert _same(one, again)
    assert not np.array_equal(one[0], plain[0]) and max(i["numRefactor"] for i in one[4]) >= 1
    assert all(i["numRefactor"] == 0 and i["rhoFinal"] == RHO and i["rhoProposed"] == RHO and i["tRefactor"] == 0 for i in plain[4] + back[4])


def _launches(prob, word):
    hit = [k for k in prob.kernel_times() if word in k["name"]]      # (a category without a sample is not listed)
    assert len(hit) <= 1, (word, [k["name"] for k in prob.kernel_times()])
    return hit[0]["launches"] if hit else 0


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
def test_resolve_at_the_last_rho_reuses_the_factor(gpu, sparse):
    """After a solve the factor belongs to the last rho: update() and solve(reuseFactor=True, ρ=rhoFinal) of the column that ran longest factorises nothing at
    setup (the profiler's "factorisation at setup" category counts them), and equals a fresh mode-1 handle started at that rho bit for bit."""
    name = "lasso10-f4" if sparse else "shared96-f3"
    P, A, Q, L, U, _, f = data(name)
    Q2 = Q[::-1].copy()
    with _make(gpu, sparse, P, A, Q, L, U) as prob:
        prob.set_adaptive_rho()
        prob.set_profiling(1)
        first = _run(prob, fctrΡ=f, **KW)
        last = max(first[4], key=lambda i: i["iterations"])
        assert _launches(prob, "factorisation at setup") == 1 and _launches(prob, "rho switch") == last["numRefactor"] == len(CASES[name]["switches"])
        prob.set_profiling(1)                                   # clears the counts
        prob.update(mQ=Q2)
        kw = dict(KW, ρ=last["rhoFinal"], numIterations=300)
        second = _run(prob, reuseFactor=True, fctrΡ=f, **kw)
        assert _launches(prob, "factorisation at setup") == 0
        prob.set_profiling(1)
        third = _run(prob, reuseFactor=True, fctrΡ=f, **KW)      # back at rho = 0.1: the factor is the last solve's, so this one factorises
        assert _launches(prob, "factorisation at setup") == 1 and len(third[3]) == len(Q)
    with _make(gpu, sparse, P, A, Q2, L, U) as fresh:
        fresh.set_adaptive_rho()
        want = _run(fresh, fctrΡ=f, **kw)
    assert _same(second, want)


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
def test_refusals(gpu, sparse):
    from quadraticprogramsolver_amd import _lib
    name = "random20-f5" if sparse else "shared96-f5"
    P, A, Q, L, U, _, f = data(name)
    kw = dict(numIterations=100, ϵAbs=0.0, ϵRel=0.0, ρ=RHO)
    with _make(gpu, sparse, P, A, Q, L, U) as prob:
        prob.set_adaptive_rho()
        ok = _run(prob, **kw)
        with pytest.raises(gpu.QpsError) as e:
            prob.solve(adptΡ=True, **kw)                          # the per-problem rule stays refused, also under mode 1
        assert e.value.status == UNSUPPORTED and "adptRho" in e.value.message
        for bad in (0.0, -1.0, float("nan")):
            with pytest.raises(gpu.QpsError) as e:
                prob.solve(fctrΡ=bad, **kw)
            assert e.value.status == BAD_ARGUMENT and "fctrRho" in e.value.message
        for mode in (2, -1):
            assert _lib.lib().qps_set_shared_adaptive_rho(prob._h, mode) == BAD_ARGUMENT
        assert _same(_run(prob, **kw), ok)                        # the handle keeps its mode and stays usable
        prob.set_adaptive_rho(False)
        prob.solve(fctrΡ=0.0, **kw)                               # fctrRho is not read under mode 0, as before
        with pytest.raises(gpu.QpsError) as e:
            prob.solve(adptΡ=True, **kw)
        assert e.value.status == UNSUPPORTED and "adptRho" in e.value.message


def test_other_handles_are_unsupported(gpu):
    from quadraticprogramsolver_amd import _lib
    P, A, Q, L, U, _, _ = data("shared96-f5")
    fn = _lib.lib().qps_set_shared_adaptive_rho
    with gpu.QuadraticProgram(P, Q[0], A, L[0], U[0]) as one:
        for mode in (0, 1):
            assert fn(one._h, mode) == UNSUPPORTED
            assert b"shared-matrix batch" in _lib.lib().qps_last_error(one._h)
        assert fn(one._h, 2) == BAD_ARGUMENT
    with gpu.QuadraticProgramBatch([(P, Q[b], A, L[b], U[b]) for b in range(2)]) as batch:
        assert fn(batch._h, 1) == UNSUPPORTED
        assert b"shared-matrix batch" in _lib.lib().qps_last_error(batch._h)
