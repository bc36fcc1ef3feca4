"""The lock-step batch of dense QPs (QuadraticProgramBatch off the one-workgroup-per-QP kernel) in every band of its count- and width-dependent launch
plans, both types: K = 20 iterations with a check every 10 at eps = 0, rho = 0.1 and non-zero warm starts, EVERY QP of the batch against the structured
fp64 reference of its own member -- tests/batch_band_cases.py holds the case table, the plan and the instantiations every case reaches, the bounds
and the figures measured on an MI355X; tests/test_batch_bands_cpu.py checks on the CPU that every case reaches what it claims, that the members of a
batch cannot be mistaken for one another and that the bugs the table targets would show.  Then the per-QP rho of a batch: both branches of
refactor_changed and QPs frozen at different checks, against c_oracle.solve per QP.  Every figure is printed before its assertion (run with -s)."""
import time

import numpy as np
import pytest

import batch_band_cases as C
import loop_param_cases as L
import width_band_cases as W

pytestmark = pytest.mark.gpu

FIXED = dict(numIterations=C.K, numItrConv=C.PERIOD, epsAbs=0.0, epsRel=0.0, rho=C.RHO, sigma=C.SIGMA, alpha=C.ALPHA)


def _solve(gpu, case, fam, order=None):
    """(X, Z, Y, infos) of one fresh handle over the members in ``order``."""
    order = list(range(case.count)) if order is None else order
    with gpu.QuadraticProgramBatch([(fam[b].dense_P(), fam[b].q, fam[b].A, fam[b].l, fam[b].u) for b in order], dtype=case.dtype) as h:
        X, flags, infos = h.solve(np.stack([fam[b].x0 for b in order]), trsvBlock=case.trsv, **L.api_kw(FIXED))
        Z, Y = h.dual()
    return X, Z.copy(), Y.copy(), infos


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_every_qp_of_the_batch_matches_its_structured_reference(gpu, case):
    t0 = time.perf_counter()
    fam = C.members(case)
    refs = [C.reference(f) for f in fam]
    t1 = time.perf_counter()
    X, Z, Y, infos = _solve(gpu, case, fam)
    t2 = time.perf_counter()
    worst, fails = {k: (0.0, 0.0, -1) for k in W.ADMM_KEYS}, []
    for b in range(case.count):
        bound = C.bounds(case, b)
        fig = W.errors(dict(x=X[b], z=Z[b], y=Y[b], resPrim=infos[b]["resPrim"], resDual=infos[b]["resDual"]), refs[b], W.ADMM_KEYS)
        if case.count <= 20:
            print(f"batch {case.key} QP {b}: " + " ".join(f"{k} {v:.2e}/{bound[k]:.1e}" for k, v in fig.items()))
        for k, v in fig.items():
            if v / bound[k] >= worst[k][0] / max(worst[k][1], 1e-300):
                worst[k] = (v, bound[k], b)
            if not v <= bound[k]:
                fails.append((b, k, v, bound[k]))
        i = infos[b]
        if not (i["iterations"] == C.K and i["convFlag"] == 1 and i["sweepVariant"] == case.variant and i["trsvBlock"] == case.nb and i["numRefactor"] == 0):
            fails.append((b, "report", i))
    print(f"batch {case.key} worst: " + " ".join(f"{k} {v:.2e}/{bd:.1e} (QP {b})" for k, (v, bd, b) in worst.items())
          + f"; reference {t1 - t0:.1f} s, handle and solve {t2 - t1:.1f} s, wall {time.perf_counter() - t0:.1f} s")
    assert not fails, (case.key, fails[:8], len(fails))


@pytest.mark.parametrize("key", C.POSITION_KEYS)
def test_a_qp_does_not_depend_on_its_position_in_the_batch(gpu, key):
    """Every sum of the pass, the sweeps and colsum runs in an order fixed by (NP, MP, count), and the check uses integer atomicMax: QP b of a batch
    equals QP count - 1 - b of the batch in reverse order bit for bit."""
    case = C.BY_KEY[key]
    fam = C.members(case)
    fwd = _solve(gpu, case, fam)
    rev = _solve(gpu, case, fam, order=list(range(case.count))[::-1])
    diff = {name: max(float(np.abs(a[b] - r[case.count - 1 - b]).max()) for b in range(case.count)) for name, a, r in zip("xzy", fwd[:3], rev[:3])}
    print(f"position {key}: largest difference " + " ".join(f"{k} {v:.2e}" for k, v in diff.items()))
    for b in range(case.count):
        for name, a, r in zip("xzy", fwd[:3], rev[:3]):
            assert np.array_equal(a[b], r[case.count - 1 - b]), (key, b, name, diff)
        for k in ("resPrim", "resDual"):
            assert fwd[3][b][k] == rev[3][case.count - 1 - b][k], (key, b, k)


# ---------------------------------------------------------------------------------------------------------------------
# Per-QP rho: both branches of refactor_changed, QPs frozen at different checks (which branch a case takes: the CPU guards)
# ---------------------------------------------------------------------------------------------------------------------
def _rho_batch(gpu, fam, dtype, params):
    with gpu.QuadraticProgramBatch([(f.dense_P(), f.q, f.A, f.l, f.u) for f in fam], dtype=dtype) as h:
        X, flags, infos = h.solve(np.stack([f.x0 for f in fam]), **L.api_kw(params))
        Z, Y = h.dual()
    return X, Z.copy(), Y.copy(), flags, infos


@pytest.mark.parametrize("rc", C.RHO_CASES, ids=lambda rc: rc.key)
def test_per_qp_rho_refactor_branches_and_frozen_qps_match_the_oracle(gpu, c_oracle, rc):
    t0 = time.perf_counter()
    fam = C.rho_members(rc)
    X, Z, Y, flags, infos = _rho_batch(gpu, fam, "f64", C.RHO_PARAMS)
    fails = []
    for b, f in enumerate(fam):
        io, i = C.oracle_solve(c_oracle, f, **C.RHO_PARAMS), infos[b]                        # ends at this QP's own stopping iteration
        fig = dict(x=float(np.abs(X[b] - io["x"]).max()), z=W.rel(Z[b], io["z"]), y=W.rel(Y[b], io["y"]),
                   resPrim=abs(i["resPrim"] - io["resPrim"]) / max(1.0, io["resPrim"]), resDual=abs(i["resDual"] - io["resDual"]) / max(1.0, io["resDual"]),
                   rho=abs(i["rhoFinal"] - io["rhoFinal"]) / io["rhoFinal"])
        bound = dict(x=C.ABS_DEV_THR, z=C.TOL["f64"]["z"], y=C.TOL["f64"]["y"], resPrim=1e-9, resDual=1e-9, rho=1e-9)
        print(f"rho {rc.key} QP {b}: flag {int(flags[b])}/{io['convFlag']} iterations {i['iterations']}/{io['iterations']} refactors {i['numRefactor']}/{io['numRefactor']} "
              + " ".join(f"{k} {v:.2e}/{bound[k]:.0e}" for k, v in fig.items()))
        if not (int(flags[b]) == io["convFlag"] == 3 and i["iterations"] == io["iterations"] == rc.stops[b] and i["numRefactor"] == io["numRefactor"]):
            fails.append((b, "report", int(flags[b]), i["iterations"], i["numRefactor"]))
        if io["numRefactor"] != sum(b in bs for _, bs in rc.switches):
            fails.append((b, "switches", io["numRefactor"]))
        fails += [(b, k, v, bound[k]) for k, v in fig.items() if not v <= bound[k]]
    print(f"rho {rc.key}: wall {time.perf_counter() - t0:.1f} s")
    assert not fails, (rc.key, fails)


def test_fp32_per_qp_rho_of_a_batch(gpu, c_oracle):
    """The shapes of R1 in fp32 to 1e-4: the per-QP rho array read as (T) and an fp32 batched refactor, held to what
    test_small_batch_one_workgroup_per_qp holds its fp32 run to (x within 5e-3) plus equal flags."""
    fam = C.rho_members(C.RHO_BY_KEY["R1-one-by-one"])
    X, Z, Y, flags, infos = _rho_batch(gpu, fam, "f32", C.RHO_PARAMS_F32)
    for b, f in enumerate(fam):
        io = C.oracle_solve(c_oracle, f, **C.RHO_PARAMS_F32)
        dev = float(np.abs(X[b] - io["x"]).max())
        print(f"rho fp32 QP {b}: flag {int(flags[b])}/{io['convFlag']} iterations {infos[b]['iterations']}/{io['iterations']} refactors {infos[b]['numRefactor']}/{io['numRefactor']} x {dev:.2e}/5e-03")
        assert int(flags[b]) == io["convFlag"] and dev <= 5e-3, (b, int(flags[b]), io["convFlag"], dev)
