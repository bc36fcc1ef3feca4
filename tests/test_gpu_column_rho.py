"""Per-column adaptive rho on the matrix-free CG shared-matrix batch (qps_set_shared_column_rho) on the device: every column of a batch behaves as a stand-alone
solve of the C oracle's matrix-free CG plugin (KIND_CG_MATFREE) with adptRho -- its own switches, its own final rho -- and as the numpy restatement of
tests/column_rho_cases.py where an option the oracle does not have is composed with it.

A column is compared where tests/test_column_rho_cpu.py found every decision of the restatement clear of its threshold (2 % for a :47 decision, 1 % for a stopping
decision; 10 % in fp32).  Tolerances: 10 x the spread the guard measured between the oracle's CG and its sparse L D L' on the same case, with the fixed-rho bounds
of tests/test_gpu_cg_shared_batch.py (1e-7, 1e-7, 1e-6) as the floor for x, z, y."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import column_rho_cases as crc
import infeasibility_cases as ic
from cg_shared_cases import EPS_PCG_TIGHT, ITR_PCG_TIGHT, LONG_N, banded_family
from test_gpu_parity import rel

pytestmark = pytest.mark.gpu

BAD_ARGUMENT, UNSUPPORTED = 1, 8
TIGHT = dict(ϵPcg=EPS_PCG_TIGHT, numItrPcg=ITR_PCG_TIGHT)
BANDED, RANDOM = "banded20-f5", "random20-f3"


@functools.lru_cache(maxsize=None)
def data(name):
    return crc.case_data(name)


def rule_kw(name, **kw):
    return dict(dict(ρ=crc.CASES[name]["rho"], fctrΡ=crc.CASES[name]["fctrRho"]), **kw)


FIELDS = ("iterations", "cgIterations", "convFlag", "numRefactor", "rhoFinal", "rhoProposed")


def _run(gpu, P, A, Q, L, U, *, rule="column", dtype="f64", scale=None, **kw):
    """(X, Z, Y, infos) of one solve on a fresh handle under ``rule``: "column", "family" or None (the fixed rho)."""
    with gpu.QuadraticProgramCgSharedBatch(P, A, Q, L, U, dtype=dtype) as prob:
        if rule == "column":
            prob.set_column_rho()
        elif rule == "family":
            prob.set_adaptive_rho()
        if scale is not None:
            prob.set_rho_scale(scale)
        X, _, infos = prob.solve(**kw)
        Z, Y = prob.dual()
    return X, Z, Y, infos


def _same(a, b, fields=FIELDS):
    (X, Z, Y, infos), (x1, z1, y1, i1) = a, b
    return (np.array_equal(X, x1) and np.array_equal(Z, z1) and np.array_equal(Y, y1)
            and [tuple(i[f] for f in fields) for i in infos] == [tuple(i[f] for f in fields) for i in i1])


def _cut(run, sl):
    return run[0][sl], run[1][sl], run[2][sl], run[3][sl]


def _against_oracle(name, run, fixed_k, gpu):
    X, Z, Y, infos = run
    keep = crc.compared(crc.case_run(name, fixed_k=fixed_k))
    tol = crc.tolerances(name, bool(fixed_k))
    orc = crc.oracle_run(name, "cg", fixed_k)
    assert len(keep) >= crc.COUNT - crc.MAX_LEFT_OUT
    for b in keep:
        xo, io = orc[b]
        fig = (abs(infos[b]["rhoFinal"] - io["rhoFinal"]) / io["rhoFinal"], rel(X[b], xo), rel(Z[b], io["z"]), rel(Y[b], io["y"]))
        print(f"{name} K={fixed_k} column {b}: flag {infos[b]['convFlag']}/{io['convFlag']} iterations {infos[b]['iterations']}/{io['iterations']} switches "
              f"{infos[b]['numRefactor']}/{io['numRefactor']} rhoFinal {infos[b]['rhoFinal']:.6g} rel rho {fig[0]:.2e} x {fig[1]:.2e} z {fig[2]:.2e} y {fig[3]:.2e}")
        assert (infos[b]["convFlag"], infos[b]["iterations"], infos[b]["numRefactor"]) == (io["convFlag"], io["iterations"], io["numRefactor"]), (name, b)
        assert all(f <= t for f, t in zip(fig, tol)), (name, b, fig, tol)
    assert len({infos[b]["rhoFinal"] for b in keep}) >= 2
    return keep


# ---------------------------------------------------------------------------------------------------------------------
# 1, 2. per column against the C oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [BANDED, RANDOM])
def test_every_column_matches_the_oracle_with_its_own_rho(gpu, c_oracle, name):
    """To eps = 1e-6 with the inner tolerance at 1e-13: n = 70, m = 139 (one strip per row, row counts that are no multiple of 16) and n = 100, m = 50 (16 and 4
    strips), 20 columns in two panels."""
    P, A, Q, L, U = data(name)
    run = _run(gpu, P, A, Q, L, U, **rule_kw(name, ϵAbs=crc.EPS, ϵRel=crc.EPS, **TIGHT))
    keep = _against_oracle(name, run, None, gpu)
    assert len({(run[3][b]["numRefactor"], run[3][b]["iterations"]) for b in keep}) >= 2


@pytest.mark.parametrize("name", [BANDED, RANDOM])
def test_fixed_k_iterates_match_the_oracle(gpu, c_oracle, name):
    P, A, Q, L, U = data(name)
    run = _run(gpu, P, A, Q, L, U, **rule_kw(name, numIterations=crc.FIXED_K, ϵAbs=0.0, ϵRel=0.0, **TIGHT))
    _against_oracle(name, run, crc.FIXED_K, gpu)
    assert all(i["convFlag"] == 1 and i["iterations"] == crc.FIXED_K for i in run[3])


# ---------------------------------------------------------------------------------------------------------------------
# 3, 4, 5. bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [BANDED, RANDOM])
def test_a_column_equals_a_batch_of_one_bit_for_bit(gpu, name):
    """With the option on, the default eps_pcg (the CG counts differ most): the rho of a column depends on nothing around it."""
    P, A, Q, L, U = data(name)
    kw = rule_kw(name, ϵAbs=crc.EPS, ϵRel=crc.EPS, numIterations=300)
    full = _run(gpu, P, A, Q, L, U, **kw)
    assert len({i["numRefactor"] for i in full[3]}) > 1 and len({i["rhoFinal"] for i in full[3]}) > 2
    for b in (3, 17):                                            # one column from each panel
        assert _same(_cut(full, slice(b, b + 1)), _run(gpu, P, A, Q[b:b + 1], L[b:b + 1], U[b:b + 1], **kw)), b
    s16 = _run(gpu, P, A, Q[:16], L[:16], U[:16], **kw)
    s17 = _run(gpu, P, A, Q[:17], L[:17], U[:17], **kw)
    assert _same(s16, _cut(s17, slice(0, 16))) and _same(s17, _cut(full, slice(0, 17)))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", [BANDED, RANDOM])
def test_on_but_never_switching_equals_off_bit_for_bit(gpu, name, dtype):
    """fctrRho = 1e12: no proposal in [1e-3, 1e6] passes :47, so every column keeps the start rho, and rho_b, 1 / rho_b from the arrays are the scalar path's rho
    and T(1) / rho."""
    P, A, Q, L, U = data(name)
    kw = dict(ρ=crc.CASES[name]["rho"], ϵAbs=crc.EPS, ϵRel=crc.EPS, numIterations=150)
    on = _run(gpu, P, A, Q, L, U, dtype=dtype, fctrΡ=crc.NEVER, **kw)
    off = _run(gpu, P, A, Q, L, U, rule=None, dtype=dtype, **kw)
    assert all(i["numRefactor"] == 0 and i["rhoFinal"] == crc.CASES[name]["rho"] for i in on[3])
    assert _same(on, off, fields=("iterations", "cgIterations", "convFlag", "numRefactor", "rhoFinal"))
    assert any(i["rhoProposed"] != crc.CASES[name]["rho"] for i in on[3])          # the rule ran: proposals were made and never taken


@pytest.mark.parametrize("name,b", [(BANDED, 2), (BANDED, 15), (RANDOM, 0)])
def test_one_column_under_the_column_rule_is_the_family_rule_bit_for_bit(gpu, name, b):
    """With one column the family's worst column is the column: both rules are the reference's adptRho loop.  banded column 2 switches seven times.
    rhoProposed is left out: at the check at which its last column stops the family rule has no running column left and keeps the previous proposal."""
    P, A, Q, L, U = data(name)
    kw = rule_kw(name, ϵAbs=crc.EPS, ϵRel=crc.EPS, numIterations=400)
    col = _run(gpu, P, A, Q[b:b + 1], L[b:b + 1], U[b:b + 1], **kw)
    fam = _run(gpu, P, A, Q[b:b + 1], L[b:b + 1], U[b:b + 1], rule="family", **kw)
    print(f"{name} column {b}: switches {col[3][0]['numRefactor']}/{fam[3][0]['numRefactor']} rhoFinal {col[3][0]['rhoFinal']!r}/{fam[3][0]['rhoFinal']!r}")
    assert col[3][0]["numRefactor"] >= 1 and _same(col, fam, fields=FIELDS[:-1])


# ---------------------------------------------------------------------------------------------------------------------
# 6. fp32
# ---------------------------------------------------------------------------------------------------------------------
def test_fixed_k_fp32(gpu, c_oracle):
    """K = 100 on the banded case; a column is compared where every decision of the restatement up to K is 10 % clear and fp32 can resolve the residual norms
    behind it (column_rho_cases.fp32_resolves; at least 10 of 20 are compared).  Tolerances of tests/test_gpu_cg_shared_batch.py::test_fixed_k_fp32.
    Of the 16 columns that are 10 % clear the second condition removes three (17, 18, 19).  Measured without it: column 18 takes one switch where the oracle
    takes two (rhoFinal 57.5 against 25.4) -- its relative dual residual at iteration 50 is 4.5e-8, below half an ulp of fp32, so the fp32 proposal it takes
    there is rounding noise."""
    P, A, Q, L, U = data(BANDED)
    keep = crc.compared_fp32(crc.case_run(BANDED, fixed_k=crc.FIXED_K), crc.FIXED_K)
    assert len(keep) >= 13
    X, Z, Y, infos = _run(gpu, P, A, Q, L, U, dtype="f32", **rule_kw(BANDED, numIterations=crc.FIXED_K, ϵAbs=0.0, ϵRel=0.0, ϵPcg=1e-5, numItrPcg=ITR_PCG_TIGHT))
    orc = crc.oracle_run(BANDED, "cg", crc.FIXED_K)
    for b in keep:
        xo, io = orc[b]
        fig = (rel(X[b], xo), rel(Z[b], io["z"]), rel(Y[b], io["y"]))
        print(f"fp32 column {b}: switches {infos[b]['numRefactor']}/{io['numRefactor']} rhoFinal {infos[b]['rhoFinal']:.6g}/{io['rhoFinal']:.6g} rel x {fig[0]:.2e} "
              f"z {fig[1]:.2e} y {fig[2]:.2e}")
        assert infos[b]["numRefactor"] == io["numRefactor"] and infos[b]["iterations"] == crc.FIXED_K, b
        assert fig[0] <= 2e-3 and fig[1] <= 2e-3 and fig[2] <= 2e-2, (b, fig)


# ---------------------------------------------------------------------------------------------------------------------
# 7. more row groups than workgroups
# ---------------------------------------------------------------------------------------------------------------------
def test_more_row_groups_than_workgroups(gpu, c_oracle):
    """banded_family at n = 33000, K = 30 from rho = 0.05: every column switches at the top of iteration 26 (the guard holds the oracle to that), so the
    per-column kernels run five iterations with rounds that find no valid row."""
    P, A, Q, L, U = banded_family(3, n=LONG_N)
    X, Z, Y, infos = _run(gpu, P, A, Q, L, U, numIterations=crc.LONG_K, ϵAbs=0.0, ϵRel=0.0, ρ=crc.LONG_RHO, fctrΡ=5.0, **TIGHT)
    tol = crc.long_tolerances()
    for b in range(3):
        xo, io = c_oracle.solve(P, Q[b], A, L[b], U[b], rho=crc.LONG_RHO, fctrRho=5.0, adptRho=True, linsys=c_oracle.KIND_CG_MATFREE, epsPcg=EPS_PCG_TIGHT,
                                numItrPcg=ITR_PCG_TIGHT, numIterations=crc.LONG_K, epsAbs=0.0, epsRel=0.0)
        fig = (abs(infos[b]["rhoFinal"] - io["rhoFinal"]) / io["rhoFinal"], rel(X[b], xo), rel(Z[b], io["z"]), rel(Y[b], io["y"]))
        print(f"banded {LONG_N} column {b}: switches {infos[b]['numRefactor']}/{io['numRefactor']} rel rho {fig[0]:.2e} x {fig[1]:.2e} z {fig[2]:.2e} y {fig[3]:.2e}")
        assert infos[b]["numRefactor"] == io["numRefactor"] == 1
        assert all(f <= t for f, t in zip(fig, tol)), (b, fig, tol)


# ---------------------------------------------------------------------------------------------------------------------
# 8. composition
# ---------------------------------------------------------------------------------------------------------------------
def _against_restatement(kind, run):
    X, Z, Y, infos = run
    cols = crc.compose_run(kind)
    keep, tol = crc.compared(cols), crc.compose_tolerances(kind)
    assert 2 in keep
    for b in keep:
        k = cols[b]
        fig = (abs(infos[b]["rhoFinal"] - k["rhoFinal"]) / k["rhoFinal"], rel(X[b], k["x"]), rel(Z[b], k["z"]), rel(Y[b], k["y"]))
        print(f"{kind} column {b}: switches {infos[b]['numRefactor']}/{k['numRefactor']} rhoFinal {infos[b]['rhoFinal']:.6g} rel rho {fig[0]:.2e} x {fig[1]:.2e} "
              f"z {fig[2]:.2e} y {fig[3]:.2e}")
        assert infos[b]["numRefactor"] == k["numRefactor"] and infos[b]["iterations"] == crc.FIXED_K, (kind, b)
        assert all(f <= t for f, t in zip(fig, tol)), (kind, b, fig, tol)
    assert sum(infos[b]["numRefactor"] > 0 for b in keep) >= 2


def test_equality_rho_scale_composes_with_the_column_rule(gpu):
    """Row i of column b runs on rho_b s_i (s_i = 1e3 on the five rows that are equalities in column 2): two roundings on the device, one in the restatement."""
    P, A, Q, L, U = data(BANDED)
    run = _run(gpu, P, A, Q, L, U, scale=crc.equality_scale(L, U), **rule_kw(BANDED, fctrΡ=crc.EQUALITY_FCTR, numIterations=crc.FIXED_K, ϵAbs=0.0, ϵRel=0.0, **TIGHT))
    _against_restatement("equality", run)


def test_warm_start_state_after_a_vector_update(gpu):
    """The second solve continues from x, z, y of the first and starts every column at params.rho again: rho is not carried across solves."""
    P, A, Q, L, U = data(BANDED)
    kw = rule_kw(BANDED, numIterations=crc.FIXED_K, ϵAbs=0.0, ϵRel=0.0, **TIGHT)
    with gpu.QuadraticProgramCgSharedBatch(P, A, Q, L, U) as prob:
        prob.set_column_rho()
        X, _, first = prob.solve(**kw)
        prob.set_warm_start("state")
        prob.update(mQ=crc.warm_q(Q))
        X, _, infos = prob.solve(X, **kw)
        Z, Y = prob.dual()
    assert any(i["numRefactor"] > 0 for i in first)
    _against_restatement("warm", (X, Z, Y, infos))


def test_infeasibility_certificates_with_the_column_rule(gpu):
    """sparse-primal-r1 of tests/infeasibility_cases.py: column 3 has no feasible point.  Under the column rule it still ends with flag 4 and a certificate that
    satisfies the rule's inequalities recomputed from the original data, and the feasible columns converge."""
    P, A, Q, L, U = ic.case_data("sparse-primal-r1")
    with gpu.QuadraticProgramCgSharedBatch(P, A, Q, L, U) as prob:
        prob.set_column_rho()
        prob.set_infeasibility(ic.EPS_INF, ic.EPS_INF)
        X, flags, infos = prob.solve(ϵAbs=crc.EPS, ϵRel=crc.EPS, ρ=1.0, fctrΡ=5.0, **TIGHT)
        DY, DX = prob.certificate()
    print("flags", [int(f) for f in flags], "iterations", [i["iterations"] for i in infos], "switches", [i["numRefactor"] for i in infos])
    want = ic.CASES["sparse-primal-r1"]["flags"]
    bad = [b for b, f in enumerate(want) if f == ic.PRIM_INFEASIBLE]
    assert bad and [b for b, f in enumerate(flags) if int(f) == ic.PRIM_INFEASIBLE] == bad
    for b in range(len(want)):
        if b in bad:
            assert ic.certificate_holds(P, A, Q[b], L[b], U[b], DY[b], DX[b], ic.PRIM_INFEASIBLE, ic.EPS_INF, ic.EPS_INF), b
        else:
            assert int(flags[b]) in (2, 3) and not DY[b].any() and not DX[b].any(), b


def test_the_option_survives_a_matrix_update(gpu):
    P, A, Q, L, U = data(RANDOM)
    kw = rule_kw(RANDOM, ϵAbs=crc.EPS, ϵRel=crc.EPS, numIterations=300)
    with gpu.QuadraticProgramCgSharedBatch(P, A, Q, L, U) as prob:
        prob.set_column_rho()
        X, _, infos = prob.solve(**kw)
        before = (X, *prob.dual(), infos)
        prob.update_matrices(mP=P, mA=A)
        X, _, infos = prob.solve(**kw)
        after = (X, *prob.dual(), infos)
    assert max(i["numRefactor"] for i in before[3]) >= 1 and _same(before, after)


# ---------------------------------------------------------------------------------------------------------------------
# 9. refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_cg_handle_solving_as_before(gpu):
    from quadraticprogramsolver_amd import _lib
    P, A, Q, L, U = data(RANDOM)
    kw = rule_kw(RANDOM, numIterations=75, ϵAbs=crc.EPS, ϵRel=crc.EPS)
    fn = _lib.lib().qps_set_shared_column_rho

    def solved(prob, **more):
        X, _, infos = prob.solve(**dict(kw, **more))
        return (X, *prob.dual(), infos)

    with gpu.QuadraticProgramCgSharedBatch(P, A, Q, L, U) as prob:
        off = solved(prob)
        prob.set_column_rho()
        on = solved(prob)
        assert max(i["numRefactor"] for i in on[3]) >= 1 and not _same(on, off)
        for bad in (2, -1):
            assert fn(prob._h, bad) == BAD_ARGUMENT and b"qps_set_shared_column_rho" in _lib.lib().qps_last_error(prob._h)
        with pytest.raises(gpu.QpsError) as e:                   # the family rule while the column rule is on
            prob.set_adaptive_rho()
        assert e.value.status == UNSUPPORTED and "qps_set_shared_column_rho off first" in e.value.message
        prob.set_adaptive_rho(False)                             # turning either off is always accepted
        for f in (0.0, -5.0, float("nan")):
            with pytest.raises(gpu.QpsError) as e:
                prob.solve(**dict(kw, fctrΡ=f))
            assert e.value.status == BAD_ARGUMENT and "fctrRho" in e.value.message
        with pytest.raises(gpu.QpsError) as e:                   # the per-problem switch of qps_params stays refused, with its old text
            prob.solve(**dict(kw, adptΡ=True))
        assert e.value.status == UNSUPPORTED and "adptRho is not supported (the columns run in lockstep on one rho" in e.value.message
        assert _same(solved(prob), on)                           # still on, still the same handle
        prob.set_column_rho(False)
        assert _same(solved(prob), off)
        prob.solve(**dict(kw, fctrΡ=0.0))                        # fctrRho is not read while both rules are off
        prob.set_adaptive_rho()
        fam = solved(prob)
        with pytest.raises(gpu.QpsError) as e:                   # the column rule while the family rule is on
            prob.set_column_rho()
        assert e.value.status == UNSUPPORTED and "qps_set_shared_adaptive_rho off first" in e.value.message
        assert _lib.lib().qps_set_shared_adaptive_rho(prob._h, 2) == BAD_ARGUMENT
        assert _same(solved(prob), fam)
        prob.set_column_rho(False)
        prob.set_adaptive_rho(False)
        assert _same(solved(prob), off)


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
def test_the_factorising_shared_handles_refuse(gpu, sparse):
    P, A, Q, L, U = data(RANDOM)
    cls = gpu.QuadraticProgramSparseSharedBatch if sparse else gpu.QuadraticProgramSharedBatch
    kw = dict(numIterations=50, ϵAbs=crc.EPS, ϵRel=crc.EPS, ρ=0.1)
    with cls(P, A, Q[:4], L[:4], U[:4]) as prob:
        X0, _, i0 = prob.solve(**kw)
        with pytest.raises(gpu.QpsError) as e:
            prob.set_column_rho()
        assert e.value.status == UNSUPPORTED and "one factor serves every column" in e.value.message and "qps_set_shared_adaptive_rho" in e.value.message
        prob.set_column_rho(False)
        X1, _, i1 = prob.solve(**kw)
        assert np.array_equal(X0, X1) and [i["iterations"] for i in i0] == [i["iterations"] for i in i1]
        prob.set_adaptive_rho()                                  # the refused call left nothing behind that excludes the family rule
        prob.solve(**kw)


def test_other_handles_are_unsupported(gpu):
    from quadraticprogramsolver_amd import _lib
    from test_gpu_proxqp import make_problem
    P, A, Q, L, U = data(RANDOM)
    Pd, Ad = (M.toarray() if sp.issparse(M) else np.asarray(M) for M in (P, A))
    fn, err = _lib.lib().qps_set_shared_column_rho, _lib.lib().qps_last_error
    with gpu.QuadraticProgram(Pd, Q[0], Ad, L[0], U[0]) as one:
        for on in (0, 1):
            assert fn(one._h, on) == UNSUPPORTED and b"shared-matrix batch" in err(one._h)
        assert fn(one._h, 2) == BAD_ARGUMENT                     # the argument is judged first
    with gpu.QuadraticProgramBatch([(Pd, Q[b], Ad, L[b], U[b]) for b in range(2)]) as batch:
        assert fn(batch._h, 1) == UNSUPPORTED and b"shared-matrix batch" in err(batch._h)
    with gpu.ProxQP(*make_problem(12, 3, 5, 7)) as prox:
        assert fn(prox._h, 1) == UNSUPPORTED and b"shared-matrix batch" in err(prox._h)
        assert fn(prox._h, 3) == BAD_ARGUMENT
