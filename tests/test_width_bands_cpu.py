"""CPU guards of tests/test_gpu_width_bands.py, on the same case table (tests/width_band_cases.py): no device needed.

  reference is right    the structured (Woodbury) ADMM reference equals c_oracle.solve, and the structured ProxQP reference equals
                        proxqp_oracle_np, on a small member of the family (n = 300) at the scalars of the GPU runs, the adaptive run included:
                        x, z, y (and s) to 1e-12.  The residuals are differences of terms as large as maxNormPrim / maxNormDual (:88-89; about 40 here,
                        the weighted columns), so two correct summation orders differ by a rounding of THOSE: they are held to 1e-12 relative to
                        max(1, that scale), the scale the reference's own stopping test weighs them by (:99-100).
  discriminating power  for every case the reference under three models of a kernel that mishandles its top chunk -- columns >= B of A ignored in
                        the row dot, in the column accumulation, entries >= B of the right-hand side ignored by the solve -- moves each of x, z, y
                        (ProxQP: x, y, z, s) by at least 10 x the bound the GPU test applies to it in that type.
  fp32 bound            the fp32 bounds come from the recorded emulation (100 x, capped by the existing fp32 bounds); the emulation is repeated
                        for n <= 4100 and must reproduce its record within a factor 3 on the vectors.
  band assertions       NP, B, the claimed instantiations, trsvBlock and the row plan of every case follow from the restated dispatch code.
  problem family        about a third of the rows sit at a bound after the 20 iterations; P is exactly symmetric and Fortran-ordered; the adaptive
                        runs do change ρ after the first check."""
import numpy as np
import pytest

import width_band_cases as W

ALL = [(c, False) for c in W.CASES] + [(c, True) for c in W.PQ_CASES]
ALL_IDS = [("pq-" if pq else "admm-") + W.case_id(c) for c, pq in ALL]


@pytest.mark.parametrize("adpt", [False, True], ids=["fixed_rho", "adaptive_rho"])
def test_structured_admm_reference_equals_the_c_oracle(c_oracle, adpt):
    f = W.small_family()
    ref = W.admm_loop(W.Structured(f), adpt=adpt, fctr=W.ADMM_FCTR)
    x, io = c_oracle.solve(f.dense_P(), f.q, f.A, f.l, f.u, vX=f.x0, numIterations=W.K, numItrConv=W.PERIOD, epsAbs=0.0, epsRel=0.0, rho=W.RHO,
                           sigma=W.SIGMA, alpha=W.ALPHA, adptRho=adpt, fctrRho=W.ADMM_FCTR)
    assert io["iterations"] == W.K and io["numRefactor"] == ref["numRefactor"] == (1 if adpt else 0)
    assert W.rel(ref["x"], x) <= 1e-12 and W.rel(ref["z"], io["z"]) <= 1e-12 and W.rel(ref["y"], io["y"]) <= 1e-12
    assert abs(ref["resPrim"] - io["resPrim"]) <= 1e-12 * max(1.0, io["maxNormPrim"])
    assert abs(ref["resDual"] - io["resDual"]) <= 1e-12 * max(1.0, io["maxNormDual"])
    # (ρ's proposal divides by the dual residual, a rounding of 1e-13 on a value of 0.03: the GPU tests hold ρ to 1e-9)
    assert abs(ref["rhoFinal"] - io["rhoFinal"]) <= 1e-10 * io["rhoFinal"] and abs(ref["rhoProposed"] - io["rhoProposed"]) <= 1e-10 * io["rhoProposed"]


@pytest.mark.parametrize("adpt", [False, True], ids=["fixed_rho", "adaptive_rho"])
def test_structured_proxqp_reference_equals_the_numpy_oracle(adpt):
    from oracle import proxqp_oracle_np as po
    f = W.small_family(pq=True)
    ref = W.proxqp_loop(W.Structured(f), adpt=adpt)
    p = po.ProxQP(f.dense_P(), f.q, f.A[:f.me], f.b, f.A[f.me:], f.dd, f.x0, f.y0, f.z0, f.s0)
    rr = po.SolveQuadraticProgramProxQP(p, numIterations=W.K, ϵAbs=0.0, ϵRel=0.0, numItrConv=W.PERIOD, ρ=W.PQ_RHO, σ=W.PQ_SIGMA, adptΡ=adpt, τ=W.PQ_TAU)
    assert not rr["Converged"] and ref["updates"] == (2 if adpt else 0)
    for k, v in (("x", p.vX), ("y", p.vY), ("z", p.vZ), ("s", p.vS)):
        assert W.rel(ref[k], v) <= 1e-12, (k, W.rel(ref[k], v))
    assert abs(ref["resPrim"] - rr["PrimalResidual"]) <= 1e-12 * max(1.0, ref["maxNormPrim"])
    assert abs(ref["resDual"] - rr["DualResidual"]) <= 1e-12 * max(1.0, ref["maxNormDual"])
    assert abs(ref["rho"] - rr["ρ"]) <= 1e-10 * rr["ρ"]


def test_the_device_matrix_is_exactly_symmetric_and_is_not_copied():
    f = W.small_family()
    P = f.dense_P()
    assert P.flags.f_contiguous and f.A.flags.f_contiguous and np.array_equal(P, P.T)
    x = f.x0
    assert np.abs(P @ x - W.Structured(f).Px(x)).max() <= 1e-13 * np.abs(P @ x).max()
    assert np.asfortranarray(P, dtype=np.float64) is P and np.asfortranarray(f.A, dtype=np.float64) is f.A     # what the wrapper calls


@pytest.mark.parametrize("case,pq", ALL, ids=ALL_IDS)
def test_band_claims_follow_from_the_dispatch_code(case, pq):
    c, vn = case, W.VN[case.dtype]
    assert c.NP == W.roundup(c.n, 64) and c.n % 64 != 0                                    # ragged inside its 64-pad
    assert (W.proxqp_route if pq else W.pass_route)(c.dtype, c.NP) == c.pass_
    assert W.sweep_route(c.dtype, c.NP) == c.sweep and W.sweep_variant(c.dtype, c.NP) == 2 and W.pick_nb(c.dtype, c.NP) == c.nb >= c.NP
    assert c.chunk == (64 * vn if c.sweep[0] == "wave" else 512 * vn) and c.B % c.chunk == 0 and c.B < c.n <= c.B + c.chunk   # B starts the top used chunk
    th, kc = c.pass_[0], c.pass_[1]
    assert c.B % (th * vn) == 0 or (c.B // (th * vn)) == (c.NP - 1) // (th * vn)          # ... of the pass too, or it lies inside the pass's top chunk
    top = (c.NP - 1) // c.chunk                                                            # index of the top used chunk of the sweep
    if c.sweep[0] == "fused":
        assert 512 * vn * (c.sweep[1] // 2 if c.sweep[1] <= 8 else (8 if c.sweep[1] == 12 else 12)) < c.NP <= 512 * vn * c.sweep[1]   # inside the claimed band
    if c.kind == "last":
        assert c.n - c.B <= 4 and top == c.sweep[1] - 1 and (c.NP - 1) // (th * vn) == kc - 1  # every chunk of sweep and pass live, 4 real columns in the top one
    else:
        band_first = {1: 0, 2: 1, 4: 2, 8: 4, 12: 8, 16: 12}[c.sweep[1]] * c.chunk
        assert c.B == band_first or c.sweep[0] == "wave"                                     # the first n of the sweep's band ...
        assert W.sweep_route(c.dtype, W.roundup(c.B, 64)) != c.sweep or c.sweep[0] == "wave"  # ... one pad earlier is another instantiation
    if c.sweep[0] == "wave":
        assert c.NP > 64 * vn * 4 and W.sweep_route(c.dtype, 64 * vn * 4) == ("wave", 4)
    m = W.PQ_ME + W.PQ_MI if pq else W.M_ROWS
    assert m == W.M_ROWS and W.roundup(m, 64) == 2176 and W.apass_plan(2176) == (12, 182) and 2176 - 181 * 12 == 4
    assert all(12 // r >= 3 for r in c.pass_[2:])                                            # buffer A, buffer B, a reload of A
    assert all(W.PQ_ME % r != 0 for r in (2, 4))                                             # the equality / inequality boundary splits a tile


def test_band_boundaries_of_the_restated_dispatch():
    """fp64 1024 / 2048 / 4096 / 8192 / 16384 and fp32 2048 / 4096 / 8192 / 16384 / 32768 for the pass; the sweep's own limits."""
    for dtype, vn in W.VN.items():
        c = 512 * vn
        assert [W.pass_route(dtype, k * c)[:2] for k in (1, 2, 4, 8, 16)] == [(512, 1), (512, 2), (512, 4), (512, 8), (1024, 8)]
        assert [W.pass_route(dtype, k * c + 64)[:2] for k in (1, 2, 4, 8)] == [(512, 2), (512, 4), (512, 8), (1024, 8)] and W.pass_route(dtype, 16 * c + 64) is None
        assert [W.proxqp_route(dtype, k * c)[1] for k in (1, 2, 4, 8)] == [1, 2, 4, 8] and W.proxqp_route(dtype, 8 * c + 64) is None
        assert W.sweep_route(dtype, 960) == ("gemv",) and W.sweep_route(dtype, 64 * vn * 8) == ("wave", 8)
        assert [W.sweep_route(dtype, k * c + 64)[1] for k in (2, 4, 8, 12)] == [4, 8, 12, 16] and W.sweep_route(dtype, 16 * c + 64) == ("gemv",)
    assert W.sweep_route("f64", 1024 + 64) == ("fused", 2, 2) and W.sweep_route("f32", 2048 + 64) == ("fused", 2, 2)
    assert [W.sweep_rb_for(kc) for kc in range(1, 9)] == [4, 2, 4, 1, 1, 1, 1, 1]          # k_trsv.hip sweep_rb_for: kc == 3 keeps the 4-row block
    assert {c.sweep for c in W.CASES if c.sweep[:2] == ("fused", 4)} == {("fused", 4, 4), ("fused", 4, 1)}   # both row blocks of <KC 4> are reached


@pytest.mark.parametrize("case,pq", ALL, ids=ALL_IDS)
def test_every_case_fails_the_three_models_of_a_mishandled_top_chunk(case, pq):
    f = W.family(case, pq)
    loop, keys = (W.proxqp_loop, ("x", "y", "z", "s")) if pq else (W.admm_loop, ("x", "z", "y"))
    ref, bound = loop(W.Structured(f)), W.bounds(case, pq)
    assert 0.2 <= ref["active"] <= 0.45, ref["active"]                                       # about a third of the rows at a bound
    for bug in (1, 2, 3):
        moved = W.errors(loop(W.Structured(f, bug)), ref, keys)
        for k in keys:
            assert moved[k] >= 10 * bound[k], (W.case_id(case), bug, k, moved[k], bound[k])


def test_adaptive_runs_change_rho_after_the_first_check():
    c = next(c for c in W.CASES if c.dtype == "f64" and c.n == W.ADAPTIVE_N)
    a = W.admm_loop(W.Structured(W.family(c)), adpt=True, fctr=W.ADMM_FCTR)
    assert a["numRefactor"] == 1 and a["rhoFinal"] > W.ADMM_FCTR * W.RHO
    c = next(c for c in W.PQ_CASES if c.dtype == "f64" and c.n == W.ADAPTIVE_N)
    p = W.proxqp_loop(W.Structured(W.family(c, True)), adpt=True)
    assert p["firstUpdate"] == W.PERIOD and p["rho"] > 2 * W.PQ_RHO                             # iterations 11 to 20 run on the new factor


def test_fp32_bounds_come_from_the_recorded_emulation():
    for c, pq in ALL:
        b = W.bounds(c, pq)
        if c.dtype == "f64":
            assert b == (W.PQ_TOL64 if pq else W.TOL["f64"])
            continue
        emu, cap = W.EMU_F32[("pq" if pq else "admm", c.n)], (W.PQ_TOL32 if pq else W.TOL["f32"])
        assert set(emu) == set(cap) == set(b)
        for k in b:
            assert b[k] == min(100 * emu[k], cap[k]) and 1e-8 < emu[k] < 1e-4, (W.case_id(c), k)


@pytest.mark.parametrize("case,pq", [(c, pq) for c, pq in ALL if c.dtype == "f32" and c.n <= 4100],
                         ids=[i for i, (c, pq) in zip(ALL_IDS, ALL) if c.dtype == "f32" and c.n <= 4100])
def test_fp32_emulation_reproduces_its_record(case, pq):
    got, rec = W.emulation_error(case, pq), W.EMU_F32[("pq" if pq else "admm", case.n)]
    for k in ("x", "y", "z") + (("s",) if pq else ()):                                       # (the residuals are single draws: see the table)
        assert rec[k] / 3 <= got[k] <= rec[k] * 3, (W.case_id(case), k, got[k], rec[k])
