"""CPU guards of tests/test_gpu_polish_bands.py, on the same case table (tests/polish_band_cases.py): no device needed.

  pattern               the fixed multiplier holds the rows the kernel's row plan makes special: row 0 and row m - 1, one workgroup's 12 rows all inactive,
                        the next one's all active with alternating sign, active rows on both sides of a workgroup boundary and of a tile boundary of
                        R = 4 and of R = 2 only; magnitudes in [0.25, 8] (fp32 keeps every sign); 536 lower and 271 upper rows, three eighths.
  reference is right    the Woodbury / Schur direct solve equals np.linalg.solve on the dense K (δ = 0 and δ = 1e-2) and polish_oracle_np.Polish on the
                        small member of the family, to 1e-12; the refinement loop restated over a product equals Polish (counts within 2 %: P x is summed otherwise), the
                        MINRES copy of the fp32 emulation returns the oracle's bits at numpy.float64.
  band assertions       NP, B and the claimed instantiation of every case follow from the restated dispatch; the band boundaries of that dispatch.
  discriminating power  on every case: K is nonsingular with fewer active rows than columns, the restatement ends with flag 0 within half its budget
                        and (fp64) reproduces the recorded distance; each bug model -- columns >= B ignored in the row dot, in the column accumulation,
                        the mask ignored on inactive rows, (run B) the δ term dropped from the multiplier block -- ends with flag != 0 within the budget
                        or moves x by >= 1000 x the fp64 bound (>= 10 x the fp32 bound).  fp32 run B fails that guard for the δ term on every case,
                        which is why RUN_B_F32 is empty.
  fp32 bound            100 x the recorded emulation error, capped by 5e-3; the emulation is repeated for n <= 4100 and the tall case.
  further cases         257 MINRES partials at m = 65540 and the last row's multiplier in the 257th; 3 x 64 loop slabs against 256 polishing slabs in
                        the batch; the batch members with every row active are nonsingular and within the MINRES budget; the chained case's budget."""
import numpy as np
import pytest

import polish_band_cases as C
import width_band_cases as W
from oracle import polish_oracle_np as PO


def test_pattern_holds_the_rows_the_row_plan_makes_special():
    y, m = C.y_pattern(), C.M_ROWS
    assert (int((y < 0).sum()), int((y > 0).sum())) == (C.N_LOWER, C.N_UPPER) and 0.33 <= (C.N_LOWER + C.N_UPPER) / m <= 0.42
    a = np.abs(y[y != 0])
    assert a.min() >= 0.25 and a.max() <= 8.0 and np.array_equal(np.sign(y.astype(np.float32)), np.sign(y))
    assert W.apass_plan(W.roundup(m, 64)) == (C.RPW, C.WGS) and all(C.apass_plan(c.dtype, c.NP, 2176) == (C.RPW, C.WGS) for c in C.CASES)
    assert y[0] < 0 and y[m - 1] > 0 and (m - 1) // C.RPW == 177                               # the last real row sits in workgroup 177 of 182
    quiet, busy = y[C.QUIET_WG * C.RPW:(C.QUIET_WG + 1) * C.RPW], y[C.BUSY_WG * C.RPW:(C.BUSY_WG + 1) * C.RPW]
    assert busy.size == 12 and np.all(quiet == 0) and np.all(busy != 0) and np.all(np.sign(busy[1:]) == -np.sign(busy[:-1]))
    e = C.EDGE_WG * C.RPW
    assert y[e - 1] != 0 and y[e] != 0 and (e - 1) // C.RPW != e // C.RPW
    t = C.TILE_ROWS
    assert all(y[r] != 0 for r in t) and len({r // C.RPW for r in t}) == 1                     # inside one workgroup (row0 of a workgroup is a multiple of 4)
    assert t[1] % 2 == 0 and t[1] % 4 != 0 and t[3] % 4 == 0                                   # 493 | 494: R = 2 only; 495 | 496: R = 4 and R = 2
    assert {np.sign(y[r]) for r in t} == {-1.0, 1.0}


def test_reference_equals_the_dense_solve_and_the_oracle():
    f = W.small_family()
    y, P = C.y_pattern(f.m), f.dense_P()
    nact = int((y != 0).sum())
    assert 40 <= nact < f.n
    for delta in (0.0, 1e-2):
        x, lam = C.direct(f, y, delta)
        xd, K = C.dense_direct(P, f.q, f.A, f.l, f.u, y, delta)
        assert W.rel(x, xd) <= 1e-12 and np.linalg.cond(K) < 1e6
    x, _ = C.direct(f, y)
    xo, fo, io = PO.Polish(P, f.q, f.A, f.l, f.u, f.x0, y, 10, 1e-6, 1e-10, 4000)
    assert fo == 0 and W.rel(xo, x) <= 1e-12
    xr, fr, counts = C.restate(f, y, "f64", "A", numItrMinres=4000)
    assert fr == 0 and abs(sum(counts) - io["minresIterations"]) <= 0.02 * sum(counts) and len(counts) == io["refinements"] == 10 and W.rel(xr, xo) <= 1e-12
    assert io["numActiveLower"] + io["numActiveUpper"] == nact
    xb, fb, _ = C.restate(f, y, "f64", "B", numItrMinres=4000)                                 # one call at δ = 1e-2 lands on the regularised solve
    assert fb == 0 and W.rel(xb, C.direct(f, y, 1e-2)[0]) <= 1e-8 and W.rel(xb, x) > 1e-4
    # the MINRES copy at numpy.float64 is the oracle's, bit for bit
    Kp, g = C.StructuredK(f, y), C.rhs_vector(f, y)
    a = PO.minres(lambda v: Kp(v, 1e-6), g, 1e-10, 4000, np.zeros(g.size))
    b = C.minres_t(lambda v: Kp(v, 1e-6), g, 1e-10, 4000, np.zeros(g.size), np.float64)
    assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]
    # the dense product (tall case) is the structured one
    t = np.concatenate([f.x0, y])
    assert np.abs(C.DenseK(P, f.A, y)(t, 1e-2) - Kp(t, 1e-2)).max() <= 1e-12


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_band_claims_follow_from_the_dispatch_code(case):
    c, chunk = case, 512 * W.VN[case.dtype]
    assert c.NP == W.roundup(c.n, 64) and c.n % 64 != 0 and C.polish_route(c.dtype, c.NP) == c.route
    assert c.B % chunk == 0 and c.n - c.B == 4                                                 # 4 real columns in the top used chunk
    top = (c.NP - 1) // chunk
    if c.kind == "fallback":
        assert c.NP > 8 * chunk and C.polish_route(c.dtype, c.NP - 64) == ("fused", 8, 2)
        return
    assert 12 // c.route[2] >= 3                                                                # buffer A, buffer B and a reload of A
    if "last" in c.kind:
        assert top == c.route[1] - 1                                                            # every chunk of the instantiation live
    if "entry" in c.kind:
        assert C.polish_route(c.dtype, W.roundup(c.B, 64)) != c.route                           # one pad earlier is another instantiation


def test_band_boundaries_and_the_set_of_instantiations():
    for dtype, vn in W.VN.items():
        c = 512 * vn
        assert [C.polish_route(dtype, k * c) for k in (1, 2, 4, 8)] == [("fused", 1, 4), ("fused", 2, 4), ("fused", 4, 4), ("fused", 8, 2)]
        assert [C.polish_route(dtype, k * c + 64)[:2] for k in (1, 2, 4)] == [("fused", 2), ("fused", 4), ("fused", 8)]
        assert C.polish_route(dtype, 8 * c + 64) == ("gemv",)
        assert {x.route for x in C.CASES if x.dtype == dtype} == {("fused", 2, 4), ("fused", 4, 4), ("fused", 8, 2), ("gemv",)}
    assert C.polish_route("f64", 1088) == ("fused", 2, 4) and C.polish_route("f64", 64) == ("fused", 1, 4) == C.polish_route("f32", 64)   # the tall case: KC 1


def _guards(key, dtype, run, ref, bugs):
    """``bugs``: {model: (x or None, flag)} of runs that got the device's budget."""
    b, factor = C.bound(dtype, key, run), 1000.0 if dtype == "f64" else 10.0
    return {bug: flag != 0 or W.rel(x, ref) >= factor * b for bug, (x, flag) in bugs.items()}


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_every_case_fails_the_bug_models(case):
    f, y, key, dtype = W.family(case), C.y_pattern(), C.case_id(case), case.dtype
    g, act = C.rhs_vector(f, y), int((y != 0).sum())
    assert act == C.N_LOWER + C.N_UPPER < case.n
    for run in "AB":
        delta = C.run_params(dtype, run)["δ"] if run == "B" else 0.0
        ref, lam = C.direct(f, y, delta)                                                        # the Cholesky factor of the Schur complement exists ...
        res = C.StructuredK(f, y)(np.concatenate([ref, lam]), 0.0) - g
        res[:f.n] += delta * ref; res[f.n:] -= delta * lam
        assert np.abs(res).max() <= 1e-10 * np.abs(g).max()                                     # ... and the direct solve satisfies the system it claims
        x, flag, counts = C.restate(f, y, dtype, run)
        its = C.ITS[(key, run)]
        assert flag == 0 and its / 2 <= max(counts) <= 2 * its, (key, run, counts)
        if dtype == "f64":
            dist = W.rel(x, ref)
            assert dist <= 1e-11 if run == "A" else C.DIST_B[key] / 3 <= dist <= 3 * C.DIST_B[key], (key, run, dist)
        bugs = {}
        for bug in (1, 2, 3) + ((4,) if run == "B" else ()):
            xb, fb, _ = C.restate(f, y, dtype, run, bug=bug, numItrMinres=4 * its)
            bugs[bug] = (xb, fb)
        held = _guards(key, dtype, run, ref, bugs)
        if dtype == "f32" and run == "B":
            assert (held[4] and all(held.values())) == (key in C.RUN_B_F32), (key, held)       # the δ guard fails: run B is fp64 only
            assert W.rel(bugs[4][0], ref) < 10 * C.bound(dtype, key, "B")
        else:
            assert all(held.values()), (key, run, held)


def test_fp32_bounds_come_from_the_recorded_emulation():
    for c in C.CASES:
        key = C.case_id(c)
        if c.dtype == "f64":
            assert C.bound("f64", key, "A") == 1e-9 and C.bound("f64", key, "B") == 100 * C.DIST_B[key] and 1e-11 < C.DIST_B[key] < 1e-8
            continue
        assert C.bound("f32", key, "A") == 100 * C.EMU_F32[(key, "A")] < C.CAP32 and 1e-8 < C.EMU_F32[(key, "A")] < 1e-5
        assert C.bound("f32", key, "B") == C.CAP32 < 100 * C.EMU_F32[(key, "B")]
    assert C.bound("f32", "tall-f32", "A") == 100 * C.EMU_F32[("tall-f32", "A")] < C.CAP32
    assert C.RUN_A["f64"] == dict(numItrPolish=10, δ=1e-6, ϵMinres=1e-10) and C.RUN_A["f32"] == dict(numItrPolish=3, δ=1e-6, ϵMinres=1e-3)
    assert all(C.RUN_B[d] == dict(C.RUN_A[d], numItrPolish=1, δ=1e-2) for d in ("f64", "f32"))                # the same ϵMinres


@pytest.mark.parametrize("case", [c for c in C.CASES if c.dtype == "f32" and c.n <= 4100], ids=C.case_id)
def test_fp32_emulation_reproduces_its_record(case):
    f, y, key = W.family(case), C.y_pattern(), C.case_id(case)
    for run in "AB":
        ref, _ = C.direct(f, y, C.run_params("f32", run)["δ"] if run == "B" else 0.0)
        x, flag, _ = C.restate(f, y, "f32", run, T=np.float32, numItrMinres=C.budget((key, "A")))
        assert flag == 0 and C.EMU_F32[(key, run)] / 3 <= W.rel(x, ref) <= 3 * C.EMU_F32[(key, run)], (key, run, W.rel(x, ref))


def test_tall_case_has_257_partials_and_needs_its_last_row():
    f, y = C.tall(), C.tall_pattern()
    NP, MP = W.roundup(f.n, 64), W.roundup(f.m, 64)
    assert (NP, MP) == (64, 65600) and C.minres_partials(NP, MP) == 257 and C.minres_partials(NP, MP - 128) == 256
    assert (NP + f.m - 1) // 256 == 256 and y[-1] != 0 and int((y != 0).sum()) == len(C.TALL_ROWS) == 30 < f.n
    assert np.array_equal(f.P, f.P.T) and C.polish_route("f64", NP) == ("fused", 1, 4)
    g, y2 = np.concatenate([-f.q, np.where(y < 0, f.l, np.where(y > 0, f.u, 0.0))]), y.copy()
    y2[-1] = 0.0
    for dtype in ("f64", "f32"):
        for run in ("AB" if dtype == "f64" else "A"):
            par, key = C.run_params(dtype, run), f"tall-{dtype}"
            delta = par["δ"] if run == "B" else 0.0
            ref, K = C.dense_direct(f.P, f.q, f.A, f.l, f.u, y, delta)
            assert np.linalg.cond(K) < 1e3
            t, flag, counts = C.refine(C.DenseK(f.P, f.A, y), g, numItrMinres=C.budget((key, run)), **par)
            assert flag == 0 and C.ITS[(key, run)] / 2 <= max(counts) <= 2 * C.ITS[(key, run)], counts
            b, factor = C.bound(dtype, key, run), 1000.0 if dtype == "f64" else 10.0
            if dtype == "f64":
                dist = W.rel(t[:f.n], ref)
                assert dist <= 1e-11 if run == "A" else C.DIST_B[key] / 3 <= dist <= 3 * C.DIST_B[key], dist
            else:
                te, fe, _ = C.refine(C.DenseK(f.P, f.A, y, np.float32), g, numItrMinres=C.budget((key, run)), **par)
                emu = W.rel(te[:f.n].astype(np.float64), ref)
                assert fe == 0 and C.EMU_F32[(key, run)] / 3 <= emu <= 3 * C.EMU_F32[(key, run)], emu
            assert W.rel(C.dense_direct(f.P, f.q, f.A, f.l, f.u, y2, delta)[0], ref) >= factor * b    # a 257th partial that went missing loses this row
            if run == "B":
                tb, fb, _ = C.refine(C.DenseK(f.P, f.A, y, bug=4), g, numItrMinres=C.budget((key, run)), **par)
                assert fb != 0 or W.rel(tb[:f.n], ref) >= factor * b


def test_batch_plan_is_smaller_than_one_polishing_plan_and_every_active_set_is_nonsingular():
    NP, MP = W.roundup(C.BATCH_N, 64), W.roundup(C.BATCH_M, 64)
    assert (NP, MP) == (2048, 1024) and C.polish_route("f64", NP) == ("fused", 2, 4)
    loop, one = C.apass_plan("f64", NP, MP, C.BATCH_COUNT), C.apass_plan("f64", NP, MP, 1)
    assert loop == (16, 64) and one == (4, 256) and C.BATCH_COUNT * loop[1] == 192 < one[1]
    assert C.BATCH_M <= C.BATCH_N / 2
    members = C.batch_members()
    assert not np.array_equal(members[0].A, members[1].A) and not np.array_equal(members[1].q, members[2].q)
    for f in members:
        yall = np.ones(f.m)                                                                    # whichever rows the rounding noise of y activates: at most all of them
        assert np.array_equal(f.dense_P(), f.dense_P().T)
        ref, lam = C.direct(f, yall)
        res = C.StructuredK(f, yall)(np.concatenate([ref, lam]), 0.0) - C.rhs_vector(f, yall)
        assert np.abs(res).max() <= 1e-10 * max(1.0, np.abs(lam).max())
        s = np.linalg.svd(f.A, compute_uv=False)
        assert s[-1] > 0.05 * s[0] / W.WEIGHT                                                  # full row rank, by a margin
        x, flag, counts = C.restate(f, yall, "f64", "A", numItrMinres=C.budget(("batch", "A")))
        assert flag == 0 and max(counts) <= 2 * C.ITS[("batch", "A")] and W.rel(x, ref) <= 1e-11, counts


def test_chained_case_converges_within_its_budget_on_the_restated_loops_state():
    case = next(c for c in C.CASES if c.dtype == "f64" and c.n == C.CHAINED_N)
    f = W.family(case)
    y = W.admm_loop(W.Structured(f))["y"]
    assert case.route[0] == "fused" and int((y != 0).sum()) < case.n
    x, flag, counts = C.restate(f, y, "f64", "A", numItrMinres=C.budget(("chained", "A")))
    assert flag == 0 and C.ITS[("chained", "A")] / 2 <= max(counts) <= 2 * C.ITS[("chained", "A")] and W.rel(x, C.direct(f, y)[0]) <= 1e-11
