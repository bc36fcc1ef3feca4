"""CPU guards of tests/test_gpu_small_bands.py, on the same case table (tests/small_band_cases.py): no device needed.

  claims          every case's claimed route equals the restated dispatch (``small_route``) of its shape, the knob-only forms under their knobs; the
                  constants of the restatement are found in the text of k_small.hip.
  coverage        over every padded shape of the domain (NP <= 512, MP <= 2048, both types) each reachable (kernel, ST, LM, J, passes) is claimed by
                  a case, each register instantiation by a single-handle case and by a batch case: a later change to the dispatch rules fails
                  here until the table follows.
  discrimination  for every single-handle case the three bug models of width_band_cases.Structured at B, and a reference whose last real row of A is
                  zero, each move a compared quantity by at least 10 x that case's bound (the row through z).
  inputs          between 10 % and 60 % of the rows sit at a bound after the K iterations, in every case and every batch member.
  fp32 bounds     come from the recorded emulation (100 x, capped by TOL["f32"]); the emulation reproduces its record within a factor 2.
  adaptive runs   the proposal of the first check leaves the fctrRho band with margin, so a refactor and a relaunch from it_begin = 10 happen; in
                  the batch exactly one member refactors, so the members' numRefactor differ.

The structured reference itself is checked against the project's oracles by tests/test_width_bands_cpu.py."""
import os
import re

import numpy as np
import pytest

import small_band_cases as S

IDS = [S.case_id(c) for c in S.SINGLE_CASES]
# (ST, LM, J of the n-wide products, passes of A x~) of k_admm_small over the whole domain
LDS_SIGNATURES = {
    "f64": {(512, 1, 64, None), (512, 0, 64, 1), (512, 0, 64, 2), (1024, 0, 64, 2), (512, 0, 128, 1), (1024, 0, 128, 1), (512, 0, 256, 1), (512, 0, 512, 1)},
    "f32": {(512, 1, 64, None), (512, 0, 64, 1), (512, 0, 64, 2), (1024, 0, 64, 2), (512, 0, 128, 1), (1024, 0, 128, 1), (512, 0, 256, 1), (512, 0, 512, 1),
            (1024, 0, 128, 2), (1024, 0, 256, 1), (1024, 0, 512, 1)},
}


@pytest.mark.parametrize("case", S.SINGLE_CASES, ids=IDS)
def test_claimed_route_follows_from_the_dispatch_code(case):
    c = case
    assert (c.NP, c.MP) == (S.roundup(c.n, 64), S.roundup(c.m, 64)) and c.B == c.NP - 64 and S.admm_small_supported(c.dtype, c.n, c.m)
    if c.kind == "entry":
        assert (c.n, c.m) == (c.NP - 60, c.MP - 60) or (c.route[0] == "reg" and c.n == 60 and c.m == c.MP - 60)   # register NB = 1 is ragged at n = 60
    else:
        assert c.n == c.NP or c.m == c.MP
    r = S.small_route(c.dtype, c.n, c.m)
    assert S.signature(r) == c.route, (S.case_id(c), S.signature(r), c.route)
    assert (c.stream is None) == isinstance(S.member(c), S.Family) and (c.B > 0 or c.stream is not None)
    if r[0] == "lds":
        (J, G, nc), = r.n_plan
        assert J * G == r.ST and nc == c.NP <= J and (J == 64 or J // 2 < nc)
        if r.LM:
            R, parts, blocks = r.ax_plan
            assert R * parts == r.ST and blocks == -(-c.MP // R) and c.NP == 64
        else:
            assert len(r.ax_plan) == r.passes == (2 if c.MP > r.ST else 1) and all(J * G == r.ST for J, G, _ in r.ax_plan)
            if r.passes == 2:                                          # the second pass has its own J, and at a ragged shape four real entries
                assert c.kind == "full" or (r.ax_plan[1][0] == 64 != r.ax_plan[0][0] and c.m - r.ST == 4)


def test_claims_of_the_special_cases():
    """G from 16 down to 1 is reached; the last supported shape; the outside shapes; the batch rule; the knob-only forms."""
    G = {g for c in S.LDS_CASES for r in [S.small_route(c.dtype, c.n, c.m)] for _, g, _ in r.n_plan + ([] if r.LM else r.ax_plan)}
    assert G == {1, 2, 4, 8, 16}
    assert S.admm_small_supported("f64", 64, 1216) and not S.admm_small_supported("f64", 64, 1217)
    assert S.admm_small_supported("f32", 512, 64) and not S.admm_small_supported("f32", 512, 65) and S.admm_small_supported("f32", 4, 2048)
    for c in S.OUTSIDE_CASES:
        assert (c.NP, c.MP) == (S.roundup(c.n, 64), S.roundup(c.m, 64)) and S.small_route(c.dtype, c.n, c.m) is None
        assert c.NP <= S.NP_MAX and c.MP <= S.MP_MAX and S.small_lds_bytes(c.dtype, c.NP, c.MP) <= S.LDS_LIMIT     # the 1.25 MiB rule alone excludes them
    for c in S.BATCH_CASES:
        assert S.admm_small_batch_supported(c.dtype, c.n, c.m) and S.reg_instantiation(c.dtype, c.NP, c.MP) == c.route[1:]
    assert not S.admm_small_batch_supported("f64", 60, 132) and not S.admm_small_batch_supported("f32", 132, 4) and not S.admm_small_batch_supported("f32", 60, 260)
    for env, runs in S.KNOB_RUNS:
        for dtype, n, m, claim in runs:
            c = S.find(S.SINGLE_CASES, dtype, n, m)
            r = S.small_route(dtype, n, m, **S.knob_kw(env))
            assert S.signature(r) == claim != c.route, (env, dtype, n, m, S.signature(r))
    lm128 = S.small_route("f32", 68, 4, reg=False)                      # lda = 129, J = 128, G = 4
    assert lm128.LM == 1 and lm128.n_plan == [(128, 4, 128)] and lm128.ax_plan == (64, 8, 1)
    two_blocks = S.small_route("f32", 4, 260, reg=False, threads=256)   # gemv_rows_ldsmat loops over two row blocks of R = 256
    assert two_blocks.LM == 1 and two_blocks.ax_plan == (256, 1, 2)
    assert S.small_route("f64", 132, 4, reg=False, threads=256).n_plan == [(256, 1, 192)]


def test_restated_constants_stand_in_the_source():
    import quadraticprogramsolver_amd
    path = os.path.join(os.path.dirname(quadraticprogramsolver_amd.__file__), "csrc", "k_small.hip")
    with open(path, encoding="utf-8") as fh:
        src = re.sub(r"\s+", " ", fh.read())
    assert S.BYTES_LIMIT == 1.25 * 1024 * 1024 and "return bytes <= 1.25 * 1024 * 1024;" in src
    assert "const double bytes = ((double)2 * MP * NP + (double)NP * NP) * sizeof(T);" in src
    assert S.LDS_LIMIT == 150 * 1024 and "small_lds_bytes<T>(NP, MP) > 150 * 1024" in src
    assert S.LM_LIMIT == 158 * 1024 and "lm_env && (lds + small_lds_mat_bytes<T>(NP, MP) <= 158 * 1024)" in src
    assert S.ST_SWITCH == 65536 and "(int64_t)MP * NP <= 65536 ? 512 : 1024" in src
    assert S.MB_MAX == {"f64": 2, "f32": 4} and "mb_max = sizeof(T) == 8 ? 2 : 4" in src and "MP / 64 <= (sizeof(T) == 8 ? 2 : 4)" in src
    assert S.REG_NP == (64, 128) and src.count("MP >= 64 && (NP == 64 || NP == 128)") == 2      # admm_small and admm_small_batch_supported
    assert (S.NP_MAX, S.MP_MAX) == (512, 2048) and "m < 1 || NP > 512 || MP > 2048" in src
    assert "sizeof(T) * ((size_t)6 * NP + (size_t)7 * MP + 1024)" in src and "sizeof(T) * ((size_t)MP * (NP + 1) + (size_t)NP * NP)" in src
    assert "if (th <= 256) QPS_SMALL2(256, 0); else if (th <= 512) QPS_SMALL2(512, 1); else QPS_SMALL2(1024, 2);" in src
    assert "int J = 64; while (J < nc) J <<= 1;" in src and "int R = 64; while (R < nrows && R < ST) R <<= 1;" in src


def test_every_reachable_form_is_claimed_by_a_case():
    for dtype in ("f64", "f32"):
        lds, reg = set(), set()
        for NP in range(64, 513, 64):
            for MP in range(64, 2049, 64):
                r = S.small_route(dtype, NP, MP)
                if r is not None:
                    (reg if r[0] == "reg" else lds).add(S.signature(r))
                assert (r is not None and r[0] == "reg") == (S.admm_small_supported(dtype, NP, MP) and S.admm_small_batch_supported(dtype, NP, MP))
        assert {s[1:] for s in lds} == LDS_SIGNATURES[dtype]
        assert lds <= {c.route for c in S.LDS_CASES if c.dtype == dtype}, lds - {c.route for c in S.LDS_CASES if c.dtype == dtype}
        assert reg == {("reg", nb, mb) for d, nb, mb in S.REG_INSTANCES if d == dtype} and len(reg) == (4 if dtype == "f64" else 8)
        assert reg <= {c.route for c in S.REG_CASES if c.dtype == dtype} and reg == {c.route for c in S.BATCH_CASES if c.dtype == dtype}
    assert len(S.BATCH_CASES) == 12 and S.COUNT == 3


@pytest.mark.parametrize("case", S.SINGLE_CASES, ids=IDS)
def test_every_case_fails_the_models_of_a_dropped_block_and_a_dropped_row(case):
    f, ref, bound = S.member(case), S.reference(case), S.bounds(case)
    for bug in (1, 2, 3):
        moved = S.errors(S.admm_loop(S.Structured(f, bug)), ref, S.ADMM_KEYS)
        assert max(moved[k] / bound[k] for k in S.ADMM_KEYS) >= 10, (S.case_id(case), bug, moved, bound)
    moved = S.errors(S.admm_loop(S.Structured(S.without_last_row(f))), ref, S.ADMM_KEYS)
    assert moved["z"] >= 10 * bound["z"], (S.case_id(case), moved["z"], bound["z"])
    assert np.any(f.A[f.m - 1] != 0) and not f._cache.keys() & S.without_last_row(f)._cache.keys()


def test_active_share_of_every_input():
    runs = [(c, None) for c in S.SINGLE_CASES + S.OUTSIDE_CASES] + [(c, k) for c in S.BATCH_CASES for k in range(S.COUNT)]
    for c, k in runs:
        ref = S.reference(c, k)
        assert 0.1 <= ref["active"] <= 0.6, (S.emu_key(c, k), ref["active"])
        assert np.abs(S.member(c, k).x0).min() > 0                     # non-zero warm start
    for c in S.BATCH_CASES:                                            # distinct members: matrices and warm starts
        a, b = S.member(c, 0), S.member(c, 1)
        assert not np.array_equal(a.A, b.A) and not np.array_equal(a.x0, b.x0) and not np.array_equal(a.d, b.d)


def test_fp32_bounds_come_from_the_recorded_emulation():
    assert {S.emu_key(*r) for r in S.fp32_runs()} == set(S.EMU_F32)
    for c, k, ad in S.fp32_runs():
        b, emu, cap = S.bounds(c, k, ad), S.EMU_F32[S.emu_key(c, k, ad)], S.TOL["f32"]
        assert set(b) == set(emu) == set(cap) == set(S.ADMM_KEYS)
        for q in b:
            assert b[q] == min(100 * emu[q], cap[q]) and 1e-9 < emu[q] < 1e-4, (S.emu_key(c, k, ad), q)
    for c in S.SINGLE_CASES + S.BATCH_CASES + S.OUTSIDE_CASES:
        if c.dtype == "f64":
            assert S.bounds(c, 0 if c in S.BATCH_CASES else None) == S.TOL["f64"]


@pytest.mark.parametrize("run", S.fp32_runs(), ids=[S.emu_key(*r) for r in S.fp32_runs()])
def test_fp32_emulation_reproduces_its_record(run):
    got, rec = S.emulation_error(*run), S.EMU_F32[S.emu_key(*run)]
    for q in S.ADMM_KEYS:
        assert rec[q] / 2 <= got[q] <= rec[q] * 2, (S.emu_key(*run), q, got[q], rec[q])


def _first_proposal(c, k=None):
    return S.admm_loop(S.Structured(S.member(c, k)), numIterations=S.PERIOD, adpt=True, fctr=S.ADMM_FCTR)["rhoProposed"]


def test_adaptive_runs_refactor_after_the_first_check():
    routes = []
    for a in S.ADAPTIVE_SINGLE:
        c = S.find(S.SINGLE_CASES, *a)
        prop, ref = _first_proposal(c), S.reference(c, adpt=True)
        assert prop > 1.2 * S.ADMM_FCTR * S.RHO or prop * 1.2 * S.ADMM_FCTR < S.RHO, (a, prop)      # crosses the band by 20 %: fp32 decides alike
        assert ref["numRefactor"] == 1 and ref["rhoFinal"] == prop and S.errors(ref, S.reference(c), ("x",))["x"] > 1e-3
        routes.append(c.route)
    assert routes[0][:3] == ("lds", 512, 0) and routes[1][:3] == ("lds", 512, 1) and routes[2] == ("lds", 1024, 0, 64, 2)
    assert routes[3][:2] == ("reg", 2) and S.ADAPTIVE_SINGLE[3][0] == "f32" and all(a[0] == "f64" for a in S.ADAPTIVE_SINGLE[:3])
    c = S.find(S.BATCH_CASES, *S.ADAPTIVE_BATCH)
    assert c.route == ("reg", 2, 2) and c.dtype == "f64"
    props = [_first_proposal(c, k) for k in range(S.COUNT)]
    crossed = [p > S.ADMM_FCTR * S.RHO or p * S.ADMM_FCTR < S.RHO for p in props]
    assert all(abs(p / (S.ADMM_FCTR * S.RHO) - 1) > 0.05 and abs(p * S.ADMM_FCTR / S.RHO - 1) > 0.05 for p in props), props
    nref = [S.reference(c, k, adpt=True)["numRefactor"] for k in range(S.COUNT)]
    assert nref == [int(x) for x in crossed] and sorted(nref) == [0, 0, 1]                        # one member refactors, two do not


def test_repeat_and_knob_runs_name_cases_of_the_table():
    lds, reg = (S.find(S.SINGLE_CASES, *a) for a in S.REPEAT_SINGLE)
    assert lds.route[0] == "lds" and reg.route[0] == "reg"
    assert [sorted(env) for env, _ in S.KNOB_RUNS] == [["QPS_SMALL_REG"], ["QPS_SMALL_LDSMAT"], ["QPS_SMALL_REG", "QPS_SMALL_THREADS"]]
    lm = {(c.dtype, c.n, c.m) for c in S.LDS_CASES if c.route[2] == 1}
    assert {r[:3] for r in S.KNOB_RUNS[1][1]} == lm and len(lm) == 2
