"""The polishing step's masked KKT product (k_pass_pq.hip apass_kkt: MODE 2 of k_apass) in every width band, both types, and the two-GEMV fallback at
its natural size: `qps_polish` from a FIXED multiplier pattern (the active sets are its signs) and an arbitrary x, against a direct fp64 solve of the
reduced KKT system.  Run A is the default refinement (δ = 1e-6; fp32: 3 refinements to 1e-3), run B one MINRES call at δ = 1e-2 against the
regularised direct solve, which pins the -δ mask v_λ term (fp64 only: see RUN_B_F32 in the helper).  Further: the MINRES partial sums beyond one
256-wide trip (m = 65540), batch polish where one QP's pass plan has more slabs than the batch's loop plan, the chained form at a wide shape, and
polishing leaving nothing behind in a handle.  tests/polish_band_cases.py holds the case table, the restated dispatch, the pattern, the references,
the bounds and the figures measured on an MI355X; tests/test_polish_bands_cpu.py checks on the CPU that the reference is right and that every case
would fail a product that mishandled its top chunk, its mask or its δ term.  Every figure is printed before its assertion (run with -s)."""
import time

import numpy as np
import pytest

import polish_band_cases as C
import width_band_cases as W

pytestmark = pytest.mark.gpu


def _polish(h, key, dtype, run, x0, y, ref, t0, counts=None):
    """One `qps_polish` call of a run, held to the run's checks."""
    x, bound = x0.copy(), C.bound(dtype, key, run)
    rep = h.polish(x, y, numItrMinres=C.budget((key, run)), **C.run_params(dtype, run))
    err = W.rel(x, ref)
    print(f"polish {key} run {run}: flag {rep['flag']} refinements {rep['refinements']} minres {rep['minresIterations']} (budget {C.budget((key, run))} per call) "
          f"active {rep['numActiveLower']}/{rep['numActiveUpper']} x {err:.2e}/{bound:.1e} relres {rep['relres']:.1e} wall {time.perf_counter() - t0:.1f} s")
    assert rep["flag"] == 0 and rep["refinements"] == C.run_params(dtype, run)["numItrPolish"], rep
    assert (rep["numActiveLower"], rep["numActiveUpper"]) == (counts or (int((y < 0).sum()), int((y > 0).sum())))
    assert err <= bound, (key, run, err, bound)
    assert np.abs(x - x0).max() > 0.1                                   # the arbitrary x was replaced, not kept


def _fixed_solve(h, f):
    x = f.x0.copy()
    h.solve(x, numIterations=W.K, numItrConv=W.PERIOD, ϵAbs=0.0, ϵRel=0.0, ρ=W.RHO, σ=W.SIGMA, α=W.ALPHA)
    z, y = h.dual()
    return x, z.copy(), y.copy()


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_polished_x_solves_the_reduced_kkt_system(gpu, case):
    t0 = time.perf_counter()
    f, y, key = W.family(case), C.y_pattern(), C.case_id(case)
    runs = "AB" if case.dtype == "f64" or key in C.RUN_B_F32 else "A"
    refs = {run: C.direct(f, y, C.run_params(case, run)["δ"] if run == "B" else 0.0)[0] for run in runs}
    with gpu.QuadraticProgram(f.dense_P(), f.q, f.A, f.l, f.u, dtype=case.dtype) as h:
        before = _fixed_solve(h, f) if key == f"f64-n{C.LEFT_BEHIND_N}" else None
        for run in runs:
            _polish(h, key, case.dtype, run, f.x0, y, refs[run], t0, (C.N_LOWER, C.N_UPPER))
        if before:                                                      # polishing wrote `part` and the handle's x and y: the next solve must not see it
            after = _fixed_solve(h, f)
            print(f"polish {key}: fixed-K solve after polishing, max |difference| x {np.abs(after[0] - before[0]).max():.1e} z {np.abs(after[1] - before[1]).max():.1e} "
                  f"y {np.abs(after[2] - before[2]).max():.1e}")
            assert all(np.array_equal(a, b) for a, b in zip(after, before))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_minres_partials_beyond_one_trip(gpu, dtype):
    """m = 65540: N = NP + MP = 65664 is 257 partial sums, one more than a 256-thread trip of sum_partials; the last row is active and its multiplier
    lies in that 257th partial."""
    t0 = time.perf_counter()
    f, y, key = C.tall(), C.tall_pattern(), f"tall-{dtype}"
    assert C.minres_partials(W.roundup(f.n, 64), W.roundup(f.m, 64)) == 257 and y[-1] != 0
    with gpu.QuadraticProgram(f.P, f.q, f.A, f.l, f.u, dtype=dtype) as h:
        for run in ("AB" if dtype == "f64" else "A"):
            ref, _ = C.dense_direct(f.P, f.q, f.A, f.l, f.u, y, C.run_params(dtype, run)["δ"] if run == "B" else 0.0)
            _polish(h, key, dtype, run, f.x0, y, ref, t0)


def test_batch_polish_where_one_plan_outgrows_the_batch_plan(gpu):
    """count = 3, NP = 2048, MP = 1024: the loop's plan is 3 x 64 slabs, one QP's polishing pass writes 256.  Polishing does not change y, so the
    reference of every QP is the direct solve for the active sets of the y the batch returns; the same solve without polishing before and after it
    is bit-identical."""
    t0 = time.perf_counter()
    members = C.batch_members()
    with gpu.QuadraticProgramBatch([(f.dense_P(), f.q, f.A, f.l, f.u) for f in members]) as batch:
        X0, _, _ = batch.solve(**C.BATCH_PLAIN)
        Z0, Y0 = (a.copy() for a in batch.dual())
        X, _, infos = batch.solve(numItrMinres=C.budget(("batch", "A")), **C.BATCH_SOLVE)
        Z, Y = (a.copy() for a in batch.dual())
        X1, _, _ = batch.solve(**C.BATCH_PLAIN)
        Z1, Y1 = batch.dual()
    for b, f in enumerate(members):
        ref, _ = C.direct(f, Y[b])
        err = W.rel(X[b], ref)
        print(f"batch polish QP {b}: flag {infos[b]['polishFlag']} minres {infos[b]['polishIterations']} active {int((Y[b] < 0).sum())}/{int((Y[b] > 0).sum())} "
              f"x {err:.2e}/{C.TOL64_A:.1e} moved {W.rel(X[b], X0[b]):.1e} wall {time.perf_counter() - t0:.1f} s")
        assert infos[b]["polishFlag"] == 0, infos[b]
        assert err <= C.TOL64_A and W.rel(X[b], X0[b]) >= 1000 * C.TOL64_A   # the unpolished x would fail: polishing did the work
    assert np.array_equal(Y, Y0) and np.array_equal(Z, Z0)                  # polishing leaves the loop's z and y alone
    assert np.array_equal(X1, X0) and np.array_equal(Z1, Z0) and np.array_equal(Y1, Y0)


def test_chained_polish_equals_solve_then_polish_at_a_wide_shape(gpu):
    t0 = time.perf_counter()
    case = next(c for c in C.CASES if c.dtype == "f64" and c.n == C.CHAINED_N)
    f = W.family(case)
    kw = dict(numIterations=W.K, numItrConv=W.PERIOD, ϵAbs=0.0, ϵRel=0.0, ρ=W.RHO, σ=W.SIGMA, α=W.ALPHA)
    pk = dict(ϵMinres=1e-10, numItrMinres=C.budget(("chained", "A")))
    with gpu.QuadraticProgram(f.dense_P(), f.q, f.A, f.l, f.u) as h:
        x0, i0 = f.x0.copy(), {}
        h.solve(x0, info=i0, **kw)
        _, y = h.dual()
        y = y.copy()
        x1, i1 = f.x0.copy(), {}
        h.solve(x1, info=i1, polish=True, **kw, **pk)
        xs = x0.copy()
        rep = h.polish(xs, y, **pk)
    print(f"chained n {case.n}: polishFlag {i1['polishFlag']} / {rep['flag']} polishIterations {i1['polishIterations']} / {rep['minresIterations']} "
          f"active {rep['numActiveLower']}/{rep['numActiveUpper']} max |x1 - xs| {np.abs(x1 - xs).max():.1e} moved {np.abs(x1 - x0).max():.1e} "
          f"wall {time.perf_counter() - t0:.1f} s")
    assert i0["polishFlag"] == -1 and i0["polishIterations"] == 0 and i1["iterations"] == i0["iterations"] == W.K
    assert i1["polishFlag"] == rep["flag"] == 0 and i1["polishIterations"] == rep["minresIterations"]
    assert np.array_equal(x1, xs)
