"""CPU guards of tests/test_gpu_ldl_bands.py: the case table of tests/ldl_band_cases.py reaches every lane-group form of the scalar sweeps of k_ldl.hip, a
mixed-sign, an all-negative and an absent tail and a K-split Schur complement with a partial last slice -- read off ldl_analyze and pick_lpr in the
host-only build (tests/capi/layout_shim.cpp), so that a change to either that empties a band fails here by name -- and the recorded fp32 emulation
errors, from which the GPU test takes its fp32 bounds, are reproducible and small enough to discriminate.  No device needed; run with -s for the tables."""
import functools

import numpy as np
import pytest

import ldl_band_cases as B


@functools.lru_cache(maxsize=None)
def shape(name):
    case = B.find(name)
    P, _, A, _, _ = B.problem(name)
    return B.analyze(P, A, B.case_limits(case))[0]


def test_restated_pick_lpr_agrees_with_the_library():
    """Mean lengths just below, at and just above 2, 12, 96 and 1024, at row counts around the 2048-row rule of the 256-lane form."""
    checked = set()
    for rows in (1, 3, 37, 255, 256, 2047, 2048, 2049, 5000):
        for thr in (2, 12, 96, 1024):
            for nnz in (thr * rows - 1, thr * rows, thr * rows + 1):
                got = B.library_pick_lpr(nnz, rows)
                assert B.pick_lpr(nnz, rows) == got, (nnz, rows, got)
                checked.add((got, rows > 2048))
        for nnz in (0, 1, 10 ** 7, 2 ** 33):
            assert B.pick_lpr(nnz, rows) == B.library_pick_lpr(nnz, rows), (nnz, rows)
    assert B.pick_lpr(5, 0) == B.library_pick_lpr(5, 0) == 1 and B.pick_lpr(5, -1) == B.library_pick_lpr(5, -1) == 1
    assert {f for f, _ in checked} == set(B.LPRS) and (256, True) not in checked and (64, True) in checked
    assert B.pick_lpr(1025 * 2048, 2048) == 256 and B.pick_lpr(1025 * 2049, 2049) == 64


@pytest.mark.parametrize("case", B.CASES, ids=[c.name for c in B.CASES])
def test_every_case_reaches_what_it_claims(case):
    """The claim of a case (what the GPU log prints as its id) is what the analysis and the restated dispatch give for its pattern and limits."""
    sh = shape(case.name)
    fwd, bwd, tail = B.reached(sh.forms)
    assert (sh.N, sh.Ns, sh.Nt, sh.ldt, sh.levels, sh.pos, sh.neg) == case.shape, (case.name, sh[:8])
    assert (tuple(sorted(fwd)), tuple(sorted(bwd)), tail) == (case.fwd, case.bwd, case.tail), (case.name, B.describe(sh.forms))
    assert len(sh.forms["fwd"]) == max(sh.levels - 1, 0) and len(sh.forms["bwd"]) == sh.levels
    assert sh.ldt == -(-sh.Nt // 64) * 64 and sh.pos + sh.neg == sh.Nt


def test_coverage_enumeration():
    """Over the committed cases: every form of both sweeps, each at least once on a ragged level (256 lanes = one workgroup per row: no ragged form exists)
    and at least once on a level of more than one row; tail forms 16, 64 (dense300x30-tail64) and 256; a mixed-sign tail of ldt >= 128, an all-negative
    tail, no tail; a Schur complement of several K slices with a partial last one; all three strip counts over the panel cases."""
    print("\n" + B.LEGEND)
    hit = {(sweep, lpr): {"any": [], "ragged": [], "multi": []} for sweep in ("fwd", "bwd") for lpr in B.LPRS}
    tails, facts = {}, {"mixed tail, ldt >= 128": [], "all-negative tail": [], "no tail": [], "several K slices, last one partial": []}
    for c in B.CASES:
        sh = shape(c.name)
        print(B.shape_row(c.name, B.case_limits(c), sh))
        for sweep in ("fwd", "bwd"):
            for x in sh.forms[sweep]:
                h = hit[(sweep, x.lpr)]
                h["any"].append(c.name)
                if x.ragged:
                    h["ragged"].append(c.name)
                if x.rows > 1:
                    h["multi"].append(c.name)
        if sh.forms["tail"]:
            tails.setdefault(sh.forms["tail"].lpr, []).append(c.name)
        KC, slices, last = B.schur_slices(sh.ldt, sh.ntc)
        if sh.Nt == 0:
            facts["no tail"].append(c.name)
        if sh.ldt >= 128 and sh.pos > 0 and sh.neg > 0:
            facts["mixed tail, ldt >= 128"].append(c.name)
        if sh.Nt > 0 and sh.pos == 0:
            facts["all-negative tail"].append(c.name)
        if slices > 1 and 0 < last < KC:
            facts["several K slices, last one partial"].append(c.name)
    missing = [f"{sweep} LPR {lpr}: {what}" for (sweep, lpr), h in hit.items() for what in ("any", "ragged", "multi")
               if not h[what] and not (what == "ragged" and lpr == 256)]
    missing += [f"tail LPR {lpr}" for lpr in (16, 64, 256) if lpr not in tails]
    missing += [what for what, names in facts.items() if not names]
    assert not hit[("fwd", 256)]["ragged"] and not hit[("bwd", 256)]["ragged"]          # one row per workgroup: rows % 1 == 0
    spr = {}
    for name in B.PANEL_CASES:
        fm = shape(name).forms
        spr[name] = sorted({x.spr for x in fm["fwd"] + fm["bwd"]} | ({fm["tail"].spr} if fm["tail"] else set()))
        print(f"panel case {name}: SPR {spr[name]}")
    missing += [f"panel SPR {s}" for s in B.SPRS if not any(s in v for v in spr.values())]
    assert not missing, "not reached by the committed cases: " + "; ".join(missing)
    assert tails[64] == ["dense300x30-tail64"]
    assert all(c in [x.name for x in B.CASES] for c in B.REPEAT_CASES + B.PANEL_CASES + B.EMU_RECOMPUTED)


def test_banded_pattern_is_the_one_of_the_deep_tree_tests():
    """banded_problem restates _banded_problem of tests/test_gpu_ldl.py: same draws, same matrices."""
    from quadraticprogramsolver_amd.generator import make_rng
    from test_gpu_ldl import _banded_problem
    for n, bw in ((600, 5), (37, 2)):
        a, b = B.banded_problem(n, bw, make_rng(3, n)), _banded_problem(n, bw, make_rng(3, n))
        assert (a[0] != b[0]).nnz == 0 and (a[2] != b[2]).nnz == 0 and all(np.array_equal(a[k], b[k]) for k in (1, 3, 4))


def test_slice_arithmetic_restated():
    """schur_slices against k_ldl.hip by hand: ldt = 64 -> 1 tile, up to 256 slices of at least 64 columns; ldt = 256 -> 10 tiles, 76 slices."""
    assert B.schur_slices(64, 1066) == (64, 17, 42)
    assert B.schur_slices(256, 3351) == (64, 53, 23)
    assert B.schur_slices(64, 64 * 256 + 1) == (80, 205, 65)          # ceil(16385 / 256) = 65 -> KC 80
    assert B.schur_slices(8192, 10 ** 6)[0] == 4096 and B.schur_slices(0, 5) == (0, 0, 0) and B.schur_slices(64, 0) == (0, 0, 0)


def test_what_the_generator_classes_of_the_old_pair_test_reach():
    """Printed only: PAIR_CASES of tests/test_gpu_ldl.py under the default limits never run LPR = 16 in the forward sweep, 64 or 256 in either sweep and 256
    for the tail rows; the table is kept in DESIGN.md section 5."""
    print("\n" + B.LEGEND)
    fwd, bwd, tail = set(), set(), set()
    for label, sh in B.pair_case_rows():
        print(B.shape_row(label, B.DEFAULT_LIMITS, sh))
        f, b, t = B.reached(sh.forms)
        fwd |= f; bwd |= b; tail |= {t} - {None}
    print(f"union: fwd {sorted(fwd)} bwd {sorted(bwd)} tail {sorted(tail)}")


def test_reference_solves_its_system():
    """reference_solve on both of its branches (dense LU, sparse LU): residual at fp64 round-off."""
    for name in ("dense40x60", "banded600x5"):
        P, q, A, _, _ = B.problem(name)
        n = P.shape[0]
        for step, (_, rho) in enumerate(B.STEPS):
            x, z, y = B.step_inputs(name)[step]
            rhs = B.rhs_of(q, x, z, y, rho, B.SIGMA)
            sol = B.reference_solve(P, A, rho, B.SIGMA, rhs)
            K = B.kkt(P, A, rho, B.SIGMA)
            res = np.abs(K @ sol - rhs).max() / (abs(K).sum(axis=1).max() * np.abs(sol).max() + np.abs(rhs).max())
            print(f"{name} rho {rho}: scaled residual {res:.1e}")
            assert res <= 10 * np.finfo(float).eps
            rx, rz = B.reference(name, step)
            assert np.array_equal(rx, sol[:n]) and np.array_equal(rz, z + (sol[n:] - y) / rho)


def test_recorded_emulation_errors_are_small_enough_to_discriminate():
    assert sorted(B.EMU_F32) == sorted(c.name for c in B.CASES)
    for name, figs in B.EMU_F32.items():
        assert len(figs) == len(B.STEPS)
        for ex, ez in figs:
            assert 0 < ex <= B.EMU_LIMIT and 0 < ez <= B.EMU_LIMIT, (name, ex, ez)
    assert B.bounds("dense40x60", 0, "f64") == (1e-9, 1e-9)
    assert B.bounds("dense40x60", 0, "f32") == (8 * B.EMU_F32["dense40x60"][0][0], 8 * B.EMU_F32["dense40x60"][0][1])


@pytest.mark.parametrize("name", B.EMU_RECOMPUTED)
def test_emulation_reproduces_its_recorded_errors(name):
    """float32 numpy arithmetic without BLAS sums is deterministic: the two cheapest cases reproduce their constants to two significant digits."""
    got = B.emulation_errors(name)
    for step, ((ex, ez), (rx, rz)) in enumerate(zip(got, B.EMU_F32[name])):
        print(f"{name} step {step}: emulation x {ex:.3e} (recorded {rx:.2e}) z {ez:.3e} (recorded {rz:.2e})")
        assert abs(ex - rx) <= 0.05 * rx and abs(ez - rz) <= 0.05 * rz, (name, step, ex, rx, ez, rz)
