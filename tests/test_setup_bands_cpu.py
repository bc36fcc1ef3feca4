"""CPU guards of tests/test_gpu_setup_bands.py, on the same case table (tests/setup_band_cases.py): no device needed.

  exactness       for every case M and q are exact in both types, M x* == -q bit for bit (the ρ switch: M2 x* == σ x - q), |q| < 2^24; kappa(M) <= 50 for
                  n <= 640; every 64 x 64 tile of P is dense; in the breakdown cases the leading c x c block stays SPD and column c is the first to fail.
  bound           e_alg (the numpy restatement of the device's algorithm in the type) and e_ref (a LAPACK Cholesky solve in the type) recomputed for every
                  case with n <= 2112 and for n = 4096: BOUND is 8 x their maximum, or exceeds it by at most 2 x.
  detectability   the restated L and the restated A'A perturbed at one tile -- zeroed, or taken from its mirrored position -- move x by at least
                  1000 x BOUND of either type: at every lower tile for n <= 640, at the listed tiles for n = 1600.
  coverage        the union of branches(case) over the table holds every branch of the band list, both sides of every threshold; the claims of the
                  table's ``why`` column follow from the restated dispatch code, and the restated id -> tile maps deal every lower tile exactly once."""
import math

import numpy as np
import pytest

import setup_band_cases as S

SMALL = [c for c in S.SINGLE if c.n <= 640]
_e = {dt: {} for dt in S.DTYPES}                                           # tag -> (e_alg, e_ref), filled by the bound tests of the cases


def _exact(a, dtype):
    return np.array_equal(a.astype(S.NPDT[dtype]).astype(np.float64), a)


def _check_exact(pr, rhos):
    assert np.array_equal(pr.P, pr.P.T) and np.all(np.diag(pr.P) == pr.d) and pr.d == math.ceil(4 * math.sqrt(pr.n))
    assert set(np.unique(pr.P - np.diag(np.diag(pr.P)))) <= {-1.0, 0.0, 1.0} and set(np.unique(pr.A)) <= {-1.0, 0.0, 1.0}
    assert set(np.unique(np.abs(pr.xs))) <= {1.0, 2.0, 3.0} and pr.P.flags.f_contiguous and pr.A.flags.f_contiguous
    for rho in rhos:
        M, x = pr.M(rho), pr.x_for_rho(rho)
        for dt in S.DTYPES:
            T = S.NPDT[dt]
            assert _exact(M, dt) and _exact(pr.q, dt) and _exact(x, dt) and _exact(pr.AA, dt)
            rhs = T(S.SIGMA) * x.astype(T) - pr.q.astype(T)                # the device's right-hand side, in its type
            assert np.array_equal(rhs.astype(np.float64), M @ pr.xs)      # ... is M x* bit for bit
        assert np.abs(pr.q).max() < 2 ** 24 and np.abs(M @ pr.xs).max() < 2 ** 23
    nt = -(-pr.n // 64)
    for bi in range(nt):
        for bj in range(nt):
            t = pr.P[64 * bi:64 * bi + 64, 64 * bj:64 * bj + 64]
            assert np.count_nonzero(t) >= 0.5 * t.size                    # every tile of P is dense
    if pr.n <= 640:
        ev = np.linalg.eigvalsh(pr.M(S.RHO))
        assert ev[0] > 0 and ev[-1] / ev[0] <= 50, ev[-1] / ev[0]


@pytest.mark.parametrize("case", S.SINGLE, ids=S.single_id)
def test_single_systems_are_exact_in_both_types(case):
    _check_exact(S.problem(case.n, case.m), (S.RHO, S.RHO2) if case.n in S.RHO_SWITCH else (S.RHO,))


@pytest.mark.parametrize("case", S.BATCH, ids=S.batch_id)
def test_batch_systems_are_exact_in_both_types(case):
    prs = S.batch_problems(case)
    for pr in prs:
        _check_exact(pr, (S.RHO,))
    assert all(not np.array_equal(prs[0].P, pr.P) and not np.array_equal(prs[0].xs, pr.xs) for pr in prs[1:])   # different seeds per QP


@pytest.mark.parametrize("case", S.BREAKDOWN, ids=S.breakdown_id)
def test_breakdown_systems_fail_first_at_their_column(case):
    base, P = S.breakdown_problem(case)
    pr, c = base[case.qp], case.c
    assert 0 <= c < case.n and np.array_equal(base[case.qp].P[c, c], pr.d) and P[c, c] == -pr.d
    M = P + S.RHO * pr.AA
    M[np.diag_indices(case.n)] += S.SIGMA
    assert M[c, c] < 0
    if c > 0:
        assert np.linalg.eigvalsh(M[:c, :c])[0] > 1.0                       # the leading block stays SPD: columns 0 .. c - 1 factorise
        L = np.linalg.cholesky(M[:c, :c])
        assert M[c, c] - np.sum(np.linalg.solve(L, M[:c, c]) ** 2) < 0      # the pivot of column c
    assert S.chol_scratch_fits(S.roundup(case.n, 64)) == (case.n != 40)
    assert _exact(M, "f32")


def _bound_case(tag, pr, rho):
    for dt in S.DTYPES:
        if tag not in _e[dt]:
            _e[dt][tag] = S.cpu_errors(pr, dt, rho)
        ea, er = _e[dt][tag]
        print(f"{tag} {dt}: e_alg {ea:.2e} e_ref {er:.2e} bound {S.BOUND[dt]:.2e}")
        assert 8.0 * max(ea, er, S.U[dt]) <= S.BOUND[dt], (tag, dt, ea, er)


def _bound_cases():
    for tag, pr, rho in S.all_problems():
        if pr.n <= 2112 or pr.n == 4096:
            yield tag, pr, rho


@pytest.mark.parametrize("case", [c for c in S.SINGLE if c.n <= 2112 or c.n == 4096], ids=S.single_id)
def test_bound_covers_the_restated_algorithm_and_lapack_single(case):
    pr = S.problem(case.n, case.m)
    _bound_case(S.single_id(case), pr, S.RHO)
    if case.n in S.RHO_SWITCH:
        _bound_case(S.single_id(case) + "-rho2", pr, S.RHO2)


@pytest.mark.parametrize("case", S.BATCH, ids=S.batch_id)
def test_bound_covers_the_restated_algorithm_and_lapack_batch(case):
    for b, pr in enumerate(S.batch_problems(case)):
        _bound_case(f"{S.batch_id(case)}-qp{b}", pr, S.RHO)


def test_bound_is_eight_times_the_largest_error_within_a_factor_two():
    """Over every case with n <= 2112 and n = 4096 (the figures of the two tests above are reused when they ran)."""
    for tag, pr, rho in _bound_cases():
        _bound_case(tag, pr, rho)
    for dt in S.DTYPES:
        worst = max(max(ea, er) for ea, er in _e[dt].values())
        assert S.BOUND[dt] == 8.0 * max(S.E_MAX[dt]["alg"], S.E_MAX[dt]["ref"], S.U[dt])
        assert 8.0 * max(worst, S.U[dt]) <= S.BOUND[dt] <= 16.0 * max(worst, S.U[dt]), (dt, worst, S.BOUND[dt])


def _detect(pr, tiles, tag):
    nt = S.roundup(pr.n, 64) // 64
    L0 = S.factor(S.padded(pr)[0], "f64")
    need, low = 1000.0 * max(S.BOUND.values()), math.inf
    for which in ("L", "AA"):
        for (bi, bj, how) in S.perturbations(nt, tiles):
            mv = S.moved_by(pr, which, bi, bj, how, L0)
            low = min(low, mv)
            assert mv >= need, (tag, which, bi, bj, how, mv, need)
    print(f"{tag}: {2 * len(S.perturbations(nt, tiles))} perturbations, least movement {low:.2e} against {need:.2e}")


@pytest.mark.parametrize("case", SMALL, ids=S.single_id)
def test_every_tile_perturbation_is_visible_single(case):
    _detect(S.problem(case.n, case.m), S.lower_tiles(S.roundup(case.n, 64) // 64), S.single_id(case))


@pytest.mark.parametrize("case", S.BATCH, ids=S.batch_id)
def test_every_tile_perturbation_is_visible_batch(case):
    """QP 0 at every tile, the other QPs (same shape, other seeds) at the listed tiles."""
    nt = S.roundup(case.n, 64) // 64
    for b, pr in enumerate(S.batch_problems(case)):
        _detect(pr, S.lower_tiles(nt) if b == 0 else S.listed_tiles(nt, case.count), f"{S.batch_id(case)}-qp{b}")


def test_listed_tile_perturbations_are_visible_at_n1600():
    c = next(c for c in S.SINGLE if c.n == 1600)
    tiles = S.listed_tiles(25, 1)
    assert {(0, 0), (24, 24), (24, 23)} <= set(tiles)
    _detect(S.problem(c.n, c.m), tiles, "n1600")


def test_the_table_reaches_every_branch():
    got = S.table_branches()
    assert not (S.REQUIRED - got), f"branches no case reaches: {sorted(S.REQUIRED - got)}"


def test_the_claims_of_the_table_follow_from_the_dispatch_code():
    B = lambda n, dt="f64", **kw: S.branches(n, next((c.m for c in S.SINGLE + S.BATCH if c.n == n), 64), dt, **kw)
    assert [S.roundup(c.n, 64) // 64 for c in S.SINGLE] == [1, 2, 3, 4, 5, 7, 24, 25, 26, 31, 32, 33, 48, 49, 64]
    assert not S.chol_scratch_fits(64) and S.chol_scratch_fits(128)                         # the 64-column chain: NP = 64 only
    for dt in S.DTYPES:
        assert B(40, dt) >= {"chol:64col", "dbl:none", "sweep:one_block"}
        assert B(65, dt) >= {"chol:no_loop_step", "chol:nblk_even"} and S.roundup(65, 64) == 128
        assert S.chol_steps(dt, 192) == [(0, 1, 0, 0, 1)] and B(130, dt) >= {"chol:update_g1", "chol:nblk_odd_tail", "dbl:ragged"}
        assert [s[1] for s in S.chol_steps(dt, 256)] == [2] and [s[1] for s in S.chol_steps(dt, 320)] == [3, 1]
        assert [s[3] for s in S.chol_steps(dt, 1536)][:2] == [0, 0] and [s[3] for s in S.chol_steps(dt, 1600)][:2] == [1, 0] and [s[3] for s in S.chol_steps(dt, 1664)][:2] == [1, 0]
        assert (S.chol_steps(dt, 1536)[0][2], S.chol_steps(dt, 1600)[0][2]) == (252, 275)     # nt on either side of 256
        gg = lambda n, count=1: S.gemm_plan(S.roundup(n, 64), S.roundup(n, 64), False, False, True, count, 0)
        assert not gg(1984)["lower_map"] and (gg(2048)["ids"], gg(2048)["padding"]) == (528, 0) and (gg(2112)["ids"], gg(2112)["padding"]) == (568, 7)
        assert not gg(130, 3)["lower_map"] and (gg(576, 12)["ids"], gg(576, 12)["padding"]) == (48, 3) and (gg(640, 10)["ids"], gg(640, 10)["padding"]) == (56, 1)
        assert B(3072, dt) >= {"pair:ragged_ktri1", "pair:ragged_ktri2"} and "odd:ragged_ktri2" not in B(3072, dt)
        assert B(3136, dt) >= {"pair:ragged_ktri1", "odd:ragged_ktri2"} and "pair:ragged_ktri2" not in B(3136, dt)
        assert B(4096, dt) >= {"pair:full_ktri1", "pair:full_ktri2", "dbl:full_z"} and not any(b.startswith("pair:full") for b in B(3136, dt))
        for n in (1600, 3136):
            small, large = S.TRSV[n][dt][:2], S.TRSV[n][dt][2:]
            assert all(B(n, dt, trsv=nb) >= {"sweep:multi_launch", "dbl:stops_below_NP"} for nb in small)
            assert all(S.pick_nb(dt, nb, S.roundup(n, 64)) == nb for nb in small + large)
            assert B(n, dt, trsv=large[0]) >= {"premul:on"}
        assert B(1600, "f64", trsv=1024) >= {"premul:ragged_last_row"} and 1664 - 1024 == 640      # (1600 itself: 1024 + 576)
        assert B(576, dt, count=12) >= {"batch:1d_order_with_hostloop", "chol:nblk_odd_tail"} and B(640, dt, count=10) >= {"batch:1d_order_with_hostloop"}
    f64, f32 = S.chol_steps("f64", 4096), S.chol_steps("f32", 4096)
    assert f64[0][2] > 1500 and f64[0][3] == 0 and any(s[3] for s in f64) and all(s[3] == (s[2] >= 256) for s in f32)
    assert [s[1] for s in f64 if s[2] > 1500][-1] == 56 and S.roundup(3648, 64) // 64 - 2 == 55  # g >= 55 unavoided in fp64: first steps of NP >= 3648
    assert S.pick_nb("f64", 0, 3136) == 4096 and S.pick_nb("f32", 0, 640) == 1024 and S.pick_nb("f64", 0, 64) == 64
    assert "premul:on" not in S.branches(1600, 64, "f32", trsv=2048)                         # one block of 2048 covers NP = 1664: the fused sweep


def test_the_restated_tile_maps_deal_every_lower_tile_once():
    for nt in (2, 9, 10, 25, 32, 33, 64):
        nids = S.lower_tile_ids(nt)
        got = [t for t in (S.lower_tile_of(i, nids, nt) for i in range(nids)) if t is not None]
        assert sorted(got) == S.lower_tiles(nt) and nids % 8 == 0 and nids - len(got) < 8
    for g in (1, 2, 3, 22, 23, 24, 62):
        for avoid in (0, 1):
            ids = S.chol_update_ids(g, avoid)
            got = [t for t in (S.chol_update_tile_of(i, avoid, g) for i in range(ids)) if t is not None]
            assert sorted(got) == S.lower_tiles(g)[1:], (g, avoid)
            assert not avoid or all(S.chol_update_tile_of(i, 1, g) is None for i in range(0, ids, 8))
