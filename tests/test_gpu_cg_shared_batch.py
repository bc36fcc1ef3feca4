"""Matrix-free CG shared-matrix batch on the device (qps_create_csc_shared_batch_cg): every column of a family on one sparse mP and mA behaves as a
stand-alone solve of the C oracle's matrix-free CG plugin (KIND_CG_MATFREE) at a fixed rho, and -- with the inner tolerance at 1e-13 -- as the same column of
the L D L' shared handle under every option of the family.

Tolerances at fixed K are those of test_cg_path_iterates_match_oracle (fp64) and test_cg_path_column_blocked_spmv_with_several_blocks (fp32): with the inner
tolerance at 1e-13 both CG implementations solve the linear system to fp64 accuracy, the summation orders differ."""
import functools

import numpy as np
import pytest

import family_rho_cases as frc
import infeasibility_cases as ic
from cg_shared_cases import COUNT, LONG_N, EPS_PCG_TIGHT, ITR_PCG_TIGHT, RANDOM_FAMILY_ORACLE_ITERATIONS, RHO, banded_family, family as _family, polish_family
from test_gpu_parity import rel

pytestmark = pytest.mark.gpu

BAD_ARGUMENT, UNSUPPORTED = 1, 8
TIGHT = dict(ϵPcg=EPS_PCG_TIGHT, numItrPcg=ITR_PCG_TIGHT)


@functools.lru_cache(maxsize=None)
def family(name):
    return _family(name, COUNT)


_ORACLE = {}


def oracle(c_oracle, name, b, **kw):
    """One C-oracle solve per (family, column, parameters), shared by the tests of this module."""
    k = (name, b, tuple(sorted(kw.items())))
    if k not in _ORACLE:
        P, A, Q, L, U = family(name)
        _ORACLE[k] = c_oracle.solve(P, Q[b], A, L[b], U[b], rho=RHO[name], linsys=c_oracle.KIND_CG_MATFREE, epsPcg=EPS_PCG_TIGHT, numItrPcg=ITR_PCG_TIGHT, **kw)
    return _ORACLE[k]


def check_fixed_k(c_oracle, name, K, X, Z, Y, flags, infos, gpu, tols, columns=None):
    for b in (range(X.shape[0]) if columns is None else columns):
        xo, io = oracle(c_oracle, name, b, numIterations=K, epsAbs=0.0, epsRel=0.0)
        fig = (rel(X[b], xo), rel(Z[b], io["z"]), rel(Y[b], io["y"]))
        print(f"{name} K={K} column {b}: rel x {fig[0]:.2e} z {fig[1]:.2e} y {fig[2]:.2e} cgIterations {infos[b]['cgIterations']}")
        assert flags[b] == gpu.ConvergenceFlag.convNumItr and infos[b]["iterations"] == K
        assert fig[0] <= tols[0] and fig[1] <= tols[1] and fig[2] <= tols[2], (name, K, b, fig)


@pytest.mark.parametrize("name", ["random", "banded"])
def test_fixed_k_iterates_match_the_oracle_per_column(gpu, c_oracle, name):
    """eps 0, K = 25 and 50, fp64, 20 columns in two panels.  random: the operator runs 16 strips per row, A u and the right-hand side 4; banded: 1 everywhere,
    with 70 and 139 rows (no multiple of the 16 rows of a workgroup)."""
    P, A, Q, L, U = family(name)
    with gpu.QuadraticProgramCgSharedBatch(P, A, Q, L, U) as prob:
        for K in (25, 50):
            X, flags, infos = prob.solve(numIterations=K, ϵAbs=0.0, ϵRel=0.0, ρ=RHO[name], **TIGHT)
            Z, Y = prob.dual()
            assert X.shape == Q.shape and Z.shape == L.shape and Y.shape == L.shape
            check_fixed_k(c_oracle, name, K, X, Z, Y, flags, infos, gpu, (1e-7, 1e-7, 1e-6))


def test_fixed_k_fp32(gpu, c_oracle):
    P, A, Q, L, U = family("random")
    with gpu.QuadraticProgramCgSharedBatch(P, A, Q, L, U, dtype="f32") as prob:
        X, flags, infos = prob.solve(numIterations=20, ϵAbs=0.0, ϵRel=0.0, ρ=RHO["random"], ϵPcg=1e-5, numItrPcg=ITR_PCG_TIGHT)
        Z, Y = prob.dual()
    check_fixed_k(c_oracle, "random", 20, X, Z, Y, flags, infos, gpu, (2e-3, 2e-3, 2e-2))


def test_more_row_groups_than_workgroups(gpu, c_oracle):
    """banded_family at n = 33000: 2063 row groups of 16, more than the operator (2048) and the vector kernels (256) have workgroups per panel: two and nine
    rounds per workgroup, the last workgroup of each with rounds that find no valid row."""
    P, A, Q, L, U = banded_family(3, n=LONG_N)
    with gpu.QuadraticProgramCgSharedBatch(P, A, Q, L, U) as prob:
        X, flags, infos = prob.solve(numIterations=25, ϵAbs=0.0, ϵRel=0.0, ρ=1.0, **TIGHT)
        Z, Y = prob.dual()
    for b in range(3):
        xo, io = c_oracle.solve(P, Q[b], A, L[b], U[b], rho=1.0, linsys=c_oracle.KIND_CG_MATFREE, epsPcg=EPS_PCG_TIGHT, numItrPcg=ITR_PCG_TIGHT, numIterations=25,
                                epsAbs=0.0, epsRel=0.0)
        fig = (rel(X[b], xo), rel(Z[b], io["z"]), rel(Y[b], io["y"]))
        print(f"banded {LONG_N} column {b}: rel x {fig[0]:.2e} z {fig[1]:.2e} y {fig[2]:.2e}")
        assert fig[0] <= 1e-7 and fig[1] <= 1e-7 and fig[2] <= 1e-6


@pytest.mark.parametrize("name", ["random", "banded"])
def test_every_column_stops_at_its_own_iteration(gpu, c_oracle, name):
    P, A, Q, L, U = family(name)
    with gpu.QuadraticProgramCgSharedBatch(P, A, Q, L, U) as prob:
        X, flags, infos = prob.solve(ϵAbs=1e-6, ϵRel=1e-6, ρ=RHO[name], **TIGHT)
    its = []
    for b in range(COUNT):
        xo, io = oracle(c_oracle, name, b, numIterations=5000, epsAbs=1e-6, epsRel=1e-6)
        print(f"{name} column {b}: flag {int(flags[b])}/{io['convFlag']} iterations {infos[b]['iterations']}/{io['iterations']} rel x {rel(X[b], xo):.2e}")
        assert int(flags[b]) == io["convFlag"] and infos[b]["iterations"] == io["iterations"]
        assert rel(X[b], xo) <= 1e-6
        its.append(infos[b]["iterations"])
    assert len(set(its)) > 1
    if name == "random":
        assert its == RANDOM_FAMILY_ORACLE_ITERATIONS and all(int(f) == 3 for f in flags)


def _same(a, b):
    (X, Z, Y, infos), (x1, z1, y1, i1) = a, b
    return (np.array_equal(X, x1) and np.array_equal(Z, z1) and np.array_equal(Y, y1)
            and [(i["iterations"], i["cgIterations"], i["convFlag"]) for i in infos] == [(i["iterations"], i["cgIterations"], i["convFlag"]) for i in i1])


def _run(gpu, P, A, Q, L, U, **kw):
    with gpu.QuadraticProgramCgSharedBatch(P, A, Q, L, U) as prob:
        X, _, infos = prob.solve(**kw)
        Z, Y = prob.dual()
    return X, Z, Y, infos


@pytest.mark.parametrize("name", ["random", "banded"])
def test_a_column_equals_a_batch_of_one_bit_for_bit(gpu, name):
    """Columns stop at different ADMM iterations and need different CG counts; the default eps_pcg makes the CG counts differ most."""
    P, A, Q, L, U = family(name)
    kw = dict(ϵAbs=1e-6, ϵRel=1e-6, ρ=RHO[name], numIterations=300)
    X, Z, Y, infos = _run(gpu, P, A, Q, L, U, **kw)
    assert len({i["cgIterations"] for i in infos}) > 1
    for b in (3, 17):                                            # one column from each panel
        one = _run(gpu, P, A, Q[b:b + 1], L[b:b + 1], U[b:b + 1], **kw)
        assert _same((X[b:b + 1], Z[b:b + 1], Y[b:b + 1], infos[b:b + 1]), one), b
    s16 = _run(gpu, P, A, Q[:16], L[:16], U[:16], **kw)
    s17 = _run(gpu, P, A, Q[:17], L[:17], U[:17], **kw)
    assert _same(s16, (s17[0][:16], s17[1][:16], s17[2][:16], s17[3][:16]))


def test_cg_iterations_are_reported_per_column(gpu):
    P, A, Q, L, U = family("random")
    with gpu.QuadraticProgramCgSharedBatch(P, A, Q, L, U) as prob:
        _, _, infos = prob.solve(numIterations=50, ϵAbs=0.0, ϵRel=0.0, ρ=0.1)
        assert all(i["cgIterations"] > 0 for i in infos), [i["cgIterations"] for i in infos]
        _, flags, capped = prob.solve(numIterations=50, ϵAbs=0.0, ϵRel=0.0, ρ=0.1, ϵPcg=0.0, numItrPcg=3)
    print("cgIterations:", [i["cgIterations"] for i in infos], "capped:", [i["cgIterations"] for i in capped])
    assert all(i["cgIterations"] == 3 * i["iterations"] and i["iterations"] == 50 for i in capped)


def _against_ldl(gpu, data, setup, solve_kw, cg_kw=TIGHT):
    """The same option on the same family on both handles: (X, Z, Y, flags, infos, handle extras) of each."""
    P, A, Q, L, U = data
    out = []
    for cls, kw in ((gpu.QuadraticProgramSparseSharedBatch, {}), (gpu.QuadraticProgramCgSharedBatch, cg_kw)):
        with cls(P, A, Q, L, U) as prob:
            extra = setup(prob, dict(solve_kw, **kw))
            X, flags, infos = prob.solve(**solve_kw, **kw) if extra is None else extra
            Z, Y = prob.dual()
            out.append((X, Z, Y, flags, infos, prob.certificate()))
    return out


def _agree(ldl, cg, tag):
    for b in range(ldl[0].shape[0]):
        fig = (rel(cg[0][b], ldl[0][b]), rel(cg[1][b], ldl[1][b]), rel(cg[2][b], ldl[2][b]))
        print(f"{tag} column {b}: flag {int(cg[3][b])}/{int(ldl[3][b])} iterations {cg[4][b]['iterations']}/{ldl[4][b]['iterations']} rel x {fig[0]:.2e} z {fig[1]:.2e} "
              f"y {fig[2]:.2e}")
        assert int(cg[3][b]) == int(ldl[3][b]) and cg[4][b]["iterations"] == ldl[4][b]["iterations"], (tag, b)
        assert fig[0] <= 1e-7 and fig[1] <= 1e-7 and fig[2] <= 1e-6, (tag, b, fig)


def test_rho_scale_matches_the_ldl_handle(gpu):
    P, A, Q, L, U = family("banded")
    ldl, cg = _against_ldl(gpu, (P, A, Q, L, U), lambda prob, kw: prob.set_rho_scale(gpu.equality_rho_scale(L, U)), dict(ϵAbs=1e-6, ϵRel=1e-6, ρ=1.0))
    _agree(ldl, cg, "rho scale")


def test_family_rho_matches_the_ldl_handle(gpu):
    """random20-f5 of tests/family_rho_cases.py: rho switches at iterations 51 and 101 for the whole family; here the switch costs no factorisation."""
    P, A, Q, L, U, _, f = frc.case_data("random20-f5")
    ldl, cg = _against_ldl(gpu, (P, A, Q, L, U), lambda prob, kw: prob.set_adaptive_rho(), dict(ϵAbs=1e-6, ϵRel=1e-6, ρ=frc.RHO, fctrΡ=f))
    _agree(ldl, cg, "family rho")
    for b in range(COUNT):
        assert cg[4][b]["numRefactor"] == ldl[4][b]["numRefactor"] and abs(cg[4][b]["rhoFinal"] - ldl[4][b]["rhoFinal"]) <= 1e-7 * ldl[4][b]["rhoFinal"], b
    assert [i["iterations"] for i in cg[4]] == frc.CASES["random20-f5"]["iterations"] and max(i["numRefactor"] for i in cg[4]) == 2


@pytest.mark.parametrize("mode", ["state", "ax"])
def test_warm_start_matches_the_ldl_handle(gpu, mode):
    P, A, Q, L, U = family("random")
    Q2 = Q + 0.05 * np.roll(Q, 1, axis=0)

    def setup(prob, kw):
        X, _, _ = prob.solve(**kw)
        prob.set_warm_start(mode)
        prob.update(mQ=Q2)
        return prob.solve(X, **kw)

    ldl, cg = _against_ldl(gpu, (P, A, Q, L, U), setup, dict(ϵAbs=1e-6, ϵRel=1e-6, ρ=0.1))
    _agree(ldl, cg, f"warm start {mode}")


def test_infeasibility_certificates_match_the_ldl_handle(gpu):
    """sparse_primal of tests/infeasibility_cases.py at rho = 1: column 3 is primal infeasible (flag 4), the others converge."""
    data = ic.case_data("sparse-primal-r1")
    ldl, cg = _against_ldl(gpu, data, lambda prob, kw: prob.set_infeasibility(ic.EPS_INF, ic.EPS_INF), dict(ϵAbs=1e-6, ϵRel=1e-6, ρ=1.0))
    _agree(ldl, cg, "infeasibility")
    assert [int(f) for f in cg[3]] == ic.CASES["sparse-primal-r1"]["flags"]
    for k in (0, 1):
        assert rel(cg[5][k], ldl[5][k]) <= 1e-6 and (k == 1 or np.abs(cg[5][k]).max() > 0)


def test_polish_matches_the_ldl_handle(gpu):
    """On polish_family: equality rows and free rows only, so the active sets do not hang on the sign of a y of rounding-noise size (on banded_family as it
    is they do: the two handles agree to 1e-14 in x before the step and column 0 differs by 5e-2 after it, with equal polishFlag)."""
    P, A, Q, L, U = polish_family(COUNT)
    ldl, cg = _against_ldl(gpu, (P, A, Q, L, U), lambda prob, kw: prob.set_polish(), dict(ϵAbs=1e-6, ϵRel=1e-6, ρ=1.0))
    for b in range(COUNT):
        assert cg[4][b]["polishFlag"] == ldl[4][b]["polishFlag"] and int(cg[3][b]) == int(ldl[3][b]) and cg[4][b]["iterations"] == ldl[4][b]["iterations"], b
        print(f"polish column {b}: polishFlag {cg[4][b]['polishFlag']} rel x {rel(cg[0][b], ldl[0][b]):.2e}")
        assert rel(cg[0][b], ldl[0][b]) <= 1e-7, b
    assert any(i["polishFlag"] == 0 for i in cg[4])


def test_vector_update_equals_a_fresh_handle(gpu):
    P, A, Q, L, U = family("random")
    Q2 = Q[::-1].copy()
    kw = dict(numIterations=50, ϵAbs=0.0, ϵRel=0.0, ρ=0.1)
    with gpu.QuadraticProgramCgSharedBatch(P, A, Q, L, U) as prob:
        prob.solve(**kw)
        prob.update(mQ=Q2)
        Xa, _, ia = prob.solve(**kw)
        Za, Ya = prob.dual()
    fresh = _run(gpu, P, A, Q2, L, U, **kw)
    assert _same((Xa, Za, Ya, ia), fresh)


def test_a_pattern_the_ldl_handle_refuses(gpu, c_oracle, monkeypatch):
    """With the tail limited to 64 rows and one level allowed, the level-scheduled plugin refuses random_family at creation; the CG handle has no analysis."""
    P, A, Q, L, U = family("random")
    monkeypatch.setenv("QPS_LDL_MAX_TAIL", "64")
    monkeypatch.setenv("QPS_LDL_MAX_LEVELS", "1")
    with pytest.raises(gpu.QpsError) as e:
        gpu.QuadraticProgramSparseSharedBatch(P, A, Q, L, U)
    assert e.value.status == UNSUPPORTED
    with gpu.QuadraticProgramCgSharedBatch(P, A, Q, L, U) as prob:
        X, flags, infos = prob.solve(numIterations=25, ϵAbs=0.0, ϵRel=0.0, ρ=0.1, **TIGHT)
        Z, Y = prob.dual()
    check_fixed_k(c_oracle, "random", 25, X, Z, Y, flags, infos, gpu, (1e-7, 1e-7, 1e-6))


def test_refusals_leave_the_handle_usable(gpu, c_oracle):
    P, A, Q, L, U = family("random")
    kw = dict(numIterations=25, ϵAbs=0.0, ϵRel=0.0, ρ=0.1, **TIGHT)
    with gpu.QuadraticProgramCgSharedBatch(P, A, Q, L, U) as prob:
        for bad, status, word in ((dict(adptΡ=True), UNSUPPORTED, "adptRho"), (dict(polish=True), UNSUPPORTED, "polish"), (dict(linsys="ldl"), UNSUPPORTED, "linsys"),
                                  (dict(numItrPcg=0), BAD_ARGUMENT, "numItrPcg")):
            with pytest.raises(gpu.QpsError) as e:
                prob.solve(**dict(kw, **bad))
            assert e.value.status == status and word in str(e.value), (bad, str(e.value))
            X, flags, infos = prob.solve(linsys="cg", **kw)
            Z, Y = prob.dual()
            check_fixed_k(c_oracle, "random", 25, X, Z, Y, flags, infos, gpu, (1e-7, 1e-7, 1e-6), columns=(0, 19))
        with pytest.raises(gpu.QpsError) as e:
            prob.set_equilibration(10)
        assert e.value.status == UNSUPPORTED and "equilibration is not supported" in str(e.value)
        prob.set_equilibration(0)
        vD, vE = prob.equilibration()
        assert np.all(vD == 1.0) and np.all(vE == 1.0)
        X, flags, infos = prob.solve(**kw)
        Z, Y = prob.dual()
    check_fixed_k(c_oracle, "random", 25, X, Z, Y, flags, infos, gpu, (1e-7, 1e-7, 1e-6))


def test_profile_categories(gpu):
    P, A, Q, L, U = family("banded")
    with gpu.QuadraticProgramCgSharedBatch(P, A, Q, L, U) as prob:
        prob.set_profiling(2)
        prob.solve(numIterations=50, ϵAbs=0.0, ϵRel=0.0, ρ=1.0)
        kt = {k["name"]: k for k in prob.kernel_times()}
    for word in ("rhs", "CG iteration", "post + update", "check"):
        hit = [k for name, k in kt.items() if name.startswith("cg shared:") and word in name]
        assert len(hit) == 1 and hit[0]["launches"] > 0 and hit[0]["algo_bytes"] > 0, (word, sorted(kt))
