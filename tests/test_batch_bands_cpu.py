"""CPU guards of tests/test_gpu_batch_bands.py, on the same case table (tests/batch_band_cases.py): no device needed.

  restatement           at count = 1 the restated apass_plan / sweep_fused_slabs / pick_nb equal width_band_cases' single-QP restatement, and the
                        lines of the dispatch code they restate are still in the sources.
  band assertions       NP, MP, B, the pass instantiation, the pass plan, the sweep form with its slabs per QP, sweepVariant and trsvBlock of every
                        case follow from the restated dispatch; no case takes the one-workgroup-per-QP kernel; over the whole table both sides of
                        every threshold are reached.
  problem family        every tested member has a quarter of its rows at a bound after the 20 iterations; the reference of member b on the matrices of
                        member b' moves x by 1000 x the bound, every ordered pair of every case (beyond 20 QPs: all 20 iterations on 25 partners of
                        every member, the first iteration on all others; batch_band_cases.pair_columns); adding the member index changed no existing draw.
  bug models            a, b, c, d of the helper's docstring move a compared quantity of every tested member (all up to 3 QPs, five of a larger
                        batch) by 100 x its bound.
  size cap              device and host bytes of every case from the restated allocation list.
  fp32 bounds           from the recorded emulation (100 x, capped by TOL["f32"]); the emulation is repeated for n <= 2052.
  per-QP rho            the QPs that switch rho at every check and the check every QP stops at, from the oracle stepped by the check period: the branch of
                        refactor_changed each case claims, no switching, stopping or stall decision within 2 % of its threshold, stops at different checks,
                        and every QP that stops early would have left its stopping state by 1000 x the bound had it not been frozen."""
import os

import numpy as np
import pytest

import batch_band_cases as C
import width_band_cases as W

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "quadraticprogramsolver_amd", "csrc")


def _tested_members(case):
    """All members up to 3 QPs; of a larger batch the first two, one in the middle and the last two."""
    n = case.count
    return list(range(n)) if n <= C.PAIRWISE_DIRECT else [0, 1, n // 2, n - 2, n - 1]


def test_the_restatement_equals_the_single_qp_one_at_count_1():
    for dtype in ("f64", "f32"):
        for NP in range(64, 16448 + 1, 64):
            for MP in (64, 192, 320, 1024, 2176):
                if W.pass_route(dtype, NP) is None:
                    assert C.apass_plan(dtype, NP, MP, 1) is None
                    continue
                p = C.apass_plan(dtype, NP, MP, 1)
                assert (p.total, p.target) == (256, 256) and (p.rpw, p.slabs) == W.apass_plan(MP)
            nb = C.pick_nb(dtype, 0, NP)
            assert nb == W.pick_nb(dtype, NP)
            if nb < NP:                                                 # beyond the fused sweep's limit: blocks of 4096 (the single-QP table stops short of it)
                assert C.chol_sweep_variant(dtype, NP, nb) == 1 and not W.sweep_fused_supported(dtype, NP)
                continue
            assert C.chol_sweep_variant(dtype, NP, nb) == W.sweep_variant(dtype, NP)
            if W.sweep_fused_supported(dtype, NP):
                form, kc, rb, slabs = C.sweep_fused_slabs(dtype, NP, 1)
                assert ((form, kc) if form == "wave" else (form, kc, rb)) == W.sweep_route(dtype, NP)
                assert slabs == min(256, NP // 16 if form == "wave" else NP // rb)
            else:
                assert C.sweep_route(dtype, NP, nb, 1) == W.sweep_route(dtype, NP) == ("gemv",)


def test_the_restated_lines_are_still_in_the_sources():
    src = {f: open(os.path.join(CSRC, f)).read() for f in ("k_pass.hip", "k_trsv.hip", "k_small.hip", "dense_chol.h", "qps_dense_batch.hip", "k_loop.hip")}
    for f, line in (("k_pass.hip", "((kc1 && count > 1) ? 1024 : 256)"), ("k_pass.hip", "const int target = count >= total ? 1 : total / (count < 1 ? 1 : count);"),
                    ("k_pass.hip", "rpw = ((rpw + R - 1) / R) * R;"), ("k_trsv.hip", "const int per = count >= 256 ? 1 : 256 / (count < 1 ? 1 : count);"),
                    ("k_trsv.hip", "return std::max(1, std::min(per, NP / 16));"), ("k_trsv.hip", "(count <= 1 ? 256 : (kc <= 1 ? 1024 : (kc == 2 ? 512 : 256)))"),
                    ("k_trsv.hip", "const int per = count >= total ? 1 : total / count;"), ("k_trsv.hip", "return ntiles < per ? ntiles : per;"),
                    ("k_trsv.hip", "NP <= 64 * VecOf<T>::N * 8"), ("k_trsv.hip", "if (NP <= 64 * VecOf<T>::N * 4) QPS_WV(4);"),
                    ("k_small.hip", "MP >= 64 && (NP == 64 || NP == 128) && MP / 64 <= (sizeof(T) == 8 ? 2 : 4)"), ("dense_chol.h", "if (nb < NP) return 1;"),
                    ("dense_chol.h", "bw.vout = bx.mat = bs.count > 1 ? (int64_t)sweep_fused_slabs<T>(NP, bs.count) * NP : 0;"),
                    ("qps_dense_batch.hip", "const bool together = (int)changed.size() * 2 >= count;"),
                    ("qps_dense_batch.hip", "if (p.loopVariant == 0 && nblk == 1 && admm_small_batch_supported<T>(NP, MP))"), ("k_loop.hip", "constexpr int GC_RT = 32;")):
        assert line in src[f], (f, line)


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_band_claims_follow_from_the_dispatch_code(case):
    c, vn = case, C.VN[case.dtype]
    assert c.NP == C.roundup(c.n, 64) and c.MP == C.roundup(c.m, 64) and c.n % 64 != 0 and c.m % 64 != 0 and c.count > 1
    assert C.pass_route(c.dtype, c.NP) == c.pass_ and c.pass_[0] == 512
    assert C.apass_plan(c.dtype, c.NP, c.MP, c.count) == c.plan
    assert c.plan.total == (1024 if c.pass_[1] == 1 else 256) and c.plan.rpw % 4 == 0 and (c.plan.slabs - 1) * c.plan.rpw + c.plan.last == c.MP
    assert C.pick_nb(c.dtype, c.trsv, c.NP) == c.nb and C.chol_sweep_variant(c.dtype, c.NP, c.nb) == c.variant
    assert C.sweep_route(c.dtype, c.NP, c.nb, c.count) == c.sweep
    assert not (c.nb >= c.NP and C.admm_small_batch_supported(c.dtype, c.NP, c.MP))       # the lock-step loop, not the one-workgroup-per-QP kernel
    assert not C.admm_small_batch_supported("f64", c.NP, c.MP) and not C.admm_small_batch_supported("f32", c.NP, c.MP)
    if c.m == C.M:                                                                        # the last real row lies inside a workgroup; ragged last workgroup off KC 1 at count <= 3
        assert (c.m - 1) % c.plan.rpw not in (0, c.plan.rpw - 1) and (c.plan.last < c.plan.rpw or c.plan.rpw == 8)
    if c.NP >= 1024:                                                                      # (a variant 1 case keeps the B of the fused case of its NP)
        wave = W.sweep_route(c.dtype, c.NP)[0] == "wave"
        chunk = 64 * vn if wave else 512 * vn
        assert c.B % chunk == 0 and c.B < c.n <= c.B + chunk                              # B starts the top used chunk of the sweep kernel of this NP
    else:
        assert c.B == c.NP - 64 and c.B < c.n                                             # the last 64-column block
    if c.sweep[0] == "block":
        assert c.sweep[1] >= 2 and c.nb == c.trsv < c.NP
    if c.sweep[0] in ("wave", "fused"):                                                   # which side of the slab count's ``min`` decides
        form, kc, rb, slabs = C.sweep_fused_slabs(c.dtype, c.NP, c.count)
        assert slabs == c.sweep[-1] and slabs * c.NP * c.count < 2 ** 31


def test_both_sides_of_every_threshold_are_reached():
    cs = C.CASES
    plans = {c.key: c.plan for c in cs}
    assert {p.total for p in plans.values()} == {1024, 256}                                                  # one chunk wide or not
    assert any(1024 % c.count != 0 and c.plan.total == 1024 for c in cs) and any(256 % c.count == 0 and c.plan.total == 256 for c in cs)
    assert any(c.count >= c.plan.total and c.plan.slabs == 1 and c.plan.target == 1 for c in cs)             # the collapse band ...
    assert any(c.count < c.plan.total and 1 < c.plan.target <= 8 and c.plan.last != c.plan.rpw for c in cs)  # ... and few fat slabs short of it
    assert any(c.plan.rpw == 4 for c in cs) and any(c.plan.rpw > 4 and c.plan.last != c.plan.rpw for c in cs)
    for dtype in ("f64", "f32"):
        d = [c for c in cs if c.dtype == dtype]
        assert {c.pass_[1] for c in d} >= ({1, 2, 4, 8} if dtype == "f64" else {1, 2, 4})
        assert {c.variant for c in d} >= ({1, 2, 3} if dtype == "f64" else {2, 3})
        vn = C.VN[dtype]
        wave = [c for c in d if c.sweep[0] == "wave"]
        fused = [c for c in d if c.sweep[0] == "fused"]
        assert max(c.NP for c in wave) == 64 * vn * 8 or dtype == "f64"                                     # the last wave NP (fp64: 1024 is the only one)
        assert min(c.NP for c in fused) == max(64 * vn * 8, 1024) + (64 if dtype == "f32" else 128)          # the first NP past the wave kernel (fp64: n = 1092 as in the issue)
        assert {c.sweep[1] for c in wave} == ({8} if dtype == "f64" else {4, 8})
        assert {c.sweep[1:3] for c in fused} == ({(2, 2), (4, 4), (8, 1)} if dtype == "f64" else {(2, 2), (4, 4)})
    w64 = [c for c in cs if c.dtype == "f64" and c.sweep[0] == "wave"]
    assert any(c.sweep[2] == c.NP // 16 < 256 // c.count for c in w64) and any(c.sweep[2] == 256 // c.count < c.NP // 16 for c in w64)   # both sides of the min
    w32 = [c for c in cs if c.dtype == "f32" and c.sweep[0] == "wave"]
    assert any(c.sweep[2] == c.NP // 16 < 256 // c.count for c in w32) and any(c.sweep[2] == c.NP // 16 == 256 // c.count for c in w32)
    assert {c.sweep[3] == {1: 1024, 2: 512}.get(-(-c.NP // (512 * C.VN[c.dtype])), 256) // c.count for c in cs if c.sweep[0] == "fused"} == {True}
    assert {c.key for c in cs if c.key in C.POSITION_KEYS} == set(C.POSITION_KEYS) and all(C.BY_KEY[k].count == 3 and C.BY_KEY[k].dtype == "f64" for k in C.POSITION_KEYS)
    assert [C.refactor_together(range(k), 6) for k in (1, 2, 3, 4)] == [False, False, True, True] and C.refactor_together([0], 3) is False and C.refactor_together([0, 1], 3)


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_size_cap(case):
    dev, host = C.device_bytes(case.dtype, case.n, case.m, case.count), C.host_bytes(case.n, case.m, case.count)
    print(f"{case.key}: device {dev / 2 ** 30:.2f} GiB, host {host / 2 ** 30:.2f} GiB")
    assert dev <= C.DEVICE_CAP and host <= C.HOST_CAP


def test_the_member_index_changes_no_existing_draw():
    f, g = W.Family(300, 296, m=200), W.small_family()
    assert f.member is None and all(np.array_equal(getattr(f, k), getattr(g, k)) for k in ("d", "U", "A", "q", "l", "u", "x0"))
    b = W._base_draw()
    assert np.array_equal(f.A, np.asfortranarray(b["A"][:200, :300] * (np.where(np.arange(300) >= 296, W.WEIGHT, 1.0) / np.sqrt(300))[None, :]))
    m0, m1 = W.Family(300, 296, m=200, member=0, scale=1.0), W.Family(300, 296, m=200, member=1, scale=C.member_scale(1))
    assert not np.array_equal(m0.A, f.A) and np.abs(m0.A - m1.A).max() > 0.1 and len({C.member_scale(b) for b in range(1030)}) == 1030


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_members_are_distinguishable_and_every_bug_model_is_visible(case):
    fam = C.members(case)
    tested = _tested_members(case)
    refs = {b: C.reference(fam[b]) for b in tested}
    for b, r in refs.items():
        assert 0.25 <= r["active"] <= 0.65, (case.key, b, r["active"])                         # at least a quarter of the rows at a bound
    # every ordered pair: member b's vectors on member b''s matrices
    worst = np.inf
    if case.count <= C.PAIRWISE_DIRECT:
        for b in range(case.count):
            xb = C.bounds(case, b)["x"]
            for o in range(case.count):
                if o != b:
                    worst = min(worst, W.rel(W.admm_loop(W.Structured(C.crossed(fam[b], fam[o])))["x"], refs[b]["x"]) / xb)
    else:
        assert case.dtype == "f64"
        Q, L, U, X0 = (np.stack([getattr(f, k) for f in fam], axis=1) for k in ("q", "l", "u", "x0"))
        ops = [C.dense_ops(f) for f in fam]
        own = np.stack([C.dense_multi_loop(ops[o], Q[:, o:o + 1], L[:, o:o + 1], U[:, o:o + 1], X0[:, o:o + 1])[:, 0] for o in range(case.count)], axis=1)
        for b in tested:
            assert W.rel(own[:, b], refs[b]["x"]) <= 1e-9                                        # the dense restatement is the reference
        own1 = np.stack([C.first_x(ops[o], Q[:, o:o + 1], X0[:, o:o + 1])[:, 0] for o in range(case.count)], axis=1)
        scale, scale1 = np.maximum(1.0, np.abs(own).max(axis=0)), np.maximum(1.0, np.abs(own1).max(axis=0))
        for o in range(case.count):
            cols = C.pair_columns(case.count, o)
            d = np.abs(C.dense_multi_loop(ops[o], Q[:, cols], L[:, cols], U[:, cols], X0[:, cols]) - own[:, cols]).max(axis=0) / scale[cols]
            d[cols == o] = np.inf
            worst = min(worst, d.min() / C.TOL["f64"]["x"])
            if case.count > C.PAIRWISE_FULL:                                                     # every other ordered pair: the first iteration
                d = np.abs(C.first_x(ops[o], Q, X0) - own1).max(axis=0) / scale1
                d[o] = np.inf
                worst = min(worst, d.min() / C.TOL["f64"]["x"])
    print(f"{case.key}: least move of x over all pairs {worst:.2e} x the bound")
    assert worst >= 1000, (case.key, worst)
    # the bug models
    keys = ("x", "z", "y")
    for b in tested:
        f, bound, ref = fam[b], C.bounds(case, b), refs[b]
        r0, r1 = C.last_real_rows(case)
        assert r0 < r1 == case.m and np.abs(_rho_z_minus_y(ref)[r0:r1]).min() > 0                # bug b needs a non-zero rho z - y on those rows
        models = [("a", C.BugStructured(f, "a", case, other=fam[(b + 1) % case.count])), ("b", C.BugStructured(f, "b", case))]
        if C.last_sweep_range(case) is not None:
            e0, e1 = C.last_sweep_range(case)
            assert 0 <= e0 < e1 == case.n
            models.append(("c", C.BugStructured(f, "c", case)))
        else:
            assert case.sweep == ("gemv",)
        models += [(f"d{k}", W.Structured(f, k)) for k in (1, 2, 3)]
        for name, be in models:
            moved = W.errors(W.admm_loop(be), ref, keys)
            ratio = max(moved[k] / bound[k] for k in keys)
            print(f"{case.key} QP {b} bug {name}: " + " ".join(f"{k} {moved[k] / bound[k]:.1e}" for k in keys))
            assert ratio >= 100, (case.key, b, name, moved, bound)


def _rho_z_minus_y(ref):
    return C.RHO * ref["z"] - ref["y"]


def test_fp32_bounds_come_from_the_recorded_emulation():
    for c in C.CASES:
        for b in range(c.count if c.dtype == "f32" else 1):
            bd = C.bounds(c, b)
            if c.dtype == "f64":
                assert bd == C.TOL["f64"]
                continue
            emu, cap = C.EMU_F32[(c.key, b)], C.TOL["f32"]
            assert set(emu) == set(cap) == set(bd)
            for k in bd:
                assert bd[k] == min(100 * emu[k], cap[k]) and 1e-9 < emu[k] < 1e-4, (c.key, b, k)
    assert set(C.EMU_F32) == {(c.key, b) for c in C.CASES if c.dtype == "f32" for b in range(c.count)}


@pytest.mark.parametrize("case", [c for c in C.CASES if c.dtype == "f32" and c.n <= C.EMU_MAX_N], ids=C.case_id)
def test_fp32_emulation_reproduces_its_record(case):
    for b in range(case.count):
        got, rec = C.emulation_error(case, b), C.EMU_F32[(case.key, b)]
        for k in ("x", "y", "z"):                                                              # (the residuals are single draws: see width_band_cases)
            assert rec[k] / 3 <= got[k] <= rec[k] * 3, (case.key, b, k, got[k], rec[k])


# ---------------------------------------------------------------------------------------------------------------------
# Per-QP rho: which branch of refactor_changed every case takes, the margins of every decision, the frozen QPs
# ---------------------------------------------------------------------------------------------------------------------
_traces = {}


def _rho(co, rc):
    if rc.key not in _traces:
        fam = C.rho_members(rc)
        _traces[rc.key] = (fam, [C.rho_trace(co, f) for f in fam])
    return _traces[rc.key]


@pytest.mark.parametrize("rc", C.RHO_CASES, ids=lambda rc: rc.key)
def test_rho_cases_take_the_branches_they_claim_with_margin(c_oracle, rc):
    fam, traces = _rho(c_oracle, rc)
    count, dec = len(fam), [C.decisions(t) for t in traces]
    NP, MP = C.roundup(rc.n, 64), C.roundup(rc.m, 64)
    nb = C.pick_nb("f64", 0, NP)
    assert not C.admm_small_batch_supported("f64", NP, MP) and C.apass_plan("f64", NP, MP, count).slabs == (48 if rc.n == 150 else 80)   # rebuild_slabs clears slabs 1 ...
    assert C.sweep_route("f64", NP, nb, count) == (("gemv",) if rc.n == 150 else ("wave", 8, 64))
    for b, d in enumerate(dec):
        print(f"{rc.key} QP {b}: " + " ".join(f"{x['it']}:{'S' if x['switches'] else ''}{'stop' if x['stops'] else ''}({x['quotients'][0]:.2f},{x['quotients'][1]:.2f},{x['quotients'][3]:.2f},{x['quotients'][4]:.2f})" for x in d))
        assert C.margins_ok(d), (rc.key, b)                                                  # no decision within 2 % of its threshold
        assert d[-1]["stops"] and d[-1]["flag"] == 3 and d[-1]["it"] == rc.stops[b] < C.RHO_PARAMS["numIterations"]
        for k, io in enumerate(traces[b]):                                                   # ... and the stall test (:105-107) stays off by the same margin at every check
            before = C.oracle_solve(c_oracle, fam[b], **dict(C.RHO_PARAMS, epsAbs=0.0, epsRel=0.0, numIterations=io["iterations"] - 1))
            assert np.abs(io["x"] - before["x"]).max() > (1 + C.MARGIN) * 1e-2 * C.RHO_PARAMS["epsAbs"], (rc.key, b, k)   # epsAdmm = min(epsAbs, epsRel) * 1e-2 (:34)
    sw = {}
    for b, d in enumerate(dec):
        for x in d:
            if x["switches"]:
                sw.setdefault(x["it"], []).append(b)
    assert tuple(sorted((it, tuple(bs)) for it, bs in sw.items())) == rc.switches
    # a switch seen at check ``it`` is applied at the top of iteration it + 1; a QP that stops at check ``it`` is frozen from that check on
    first = rc.switches[0]
    together = [it for it, bs in rc.switches if C.refactor_together(bs, count)]
    alone_after_stop = [it for it, bs in rc.switches if len(bs) == 1 and not C.refactor_together(bs, count) and min(rc.stops) <= it]
    if rc.key.startswith("R1"):
        assert 1 <= len(first[1]) and not C.refactor_together(first[1], count)               # the QP-by-QP branch at the first switch, memset taken (slabs > 1)
        assert alone_after_stop
    else:                                                                                    # the batched branch, later a lone switch while another QP is frozen
        assert together and any(a > t for a in alone_after_stop for t in together)
    if rc.key.startswith("R2"):
        assert any(min(rc.stops) < a for a in alone_after_stop)                              # (R2: frozen at an earlier check)
    assert len(set(rc.stops)) >= 2                                                           # the QPs stop at two or more different checks ...
    last_switch = {b: max(it for it, bs in rc.switches if b in bs) for b in range(count) if any(b in bs for it, bs in rc.switches)}
    assert any(rc.stops[a] <= last_switch[b] for a in range(count) for b in last_switch if a != b)   # ... and one before the last switch of another is applied
    # a QP that was not frozen would fail: the oracle continued to the batch's last iteration has left the stopping state by 1000 x the bound
    last = max(rc.stops)
    for b in range(count):
        if rc.stops[b] < last:
            on = C.oracle_solve(c_oracle, fam[b], **dict(C.RHO_PARAMS, epsAbs=0.0, epsRel=0.0, numIterations=last))
            moved = {k: W.rel(on[k], traces[b][-1][k]) / C.TOL["f64"][k] for k in ("x", "z", "y")}
            print(f"{rc.key} QP {b} frozen at {rc.stops[b]}, continued to {last}: " + " ".join(f"{k} {v:.1e}" for k, v in moved.items()))
            assert max(moved.values()) > 1000, (rc.key, b, moved)
