"""In-place update of P and A of the shared-matrix batches on the device (qps_update_shared_matrices, qps_update_shared_matrices_csc): dense Cholesky, sparse
KKT L D L' and matrix-free CG handle.  The reference is the library itself on a fresh handle: an updated handle has to give what a handle created on the new
matrices gives, bit for bit -- ``same()`` of tests/test_gpu_warm_start.py: X, Z, Y, flags and every qps_info field but the wall times.  A stale CSR copy of the
check shows in resPrim / resDual, a stale factor input in the iterates.  Families, second matrices and run lengths: tests/matrix_update_cases.py (the staged
dense family, the lasso path and the scrambled families run 75 iterations with eps = 0; the others run to 1e-6, where tests/test_matrix_update_cpu.py holds the
restatement's iteration counts clear of numIterations)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import cg_shared_cases as cc
import equilibration_cases as ec
import infeasibility_cases as ic
import matrix_update_cases as mc
from test_gpu_warm_start import run, same

pytestmark = pytest.mark.gpu

BAD_ARGUMENT, NOT_FINITE, UNSUPPORTED = 1, 3, 8
CLASSES = {"dense": "QuadraticProgramSharedBatch", "sparse": "QuadraticProgramSparseSharedBatch", "cg": "QuadraticProgramCgSharedBatch"}
ONE_PER_KIND = [mc.CACHED, mc.RANDOM, mc.CG_BANDED]


def make(gpu, key, kP=0, kA=0, dtype="f64"):
    _, _, Q, L, U = mc.data(key)
    return getattr(gpu, CLASSES[mc.kind_of(key)])(mc.matrices(key, kP)[0], mc.matrices(key, kA)[1], Q, L, U, dtype=dtype)


_FRESH = {}


def fresh(gpu, key, kP, kA, dtype="f64"):
    """The cold solve of a handle created on (P_kP, A_kA), computed once and shared; nobody changes what it returns."""
    k = (key, kP, kA, dtype)
    if k not in _FRESH:
        with make(gpu, key, kP, kA, dtype) as h:
            _FRESH[k] = run(h, **mc.solve_kw(key))
    return _FRESH[k]


def differ(a, b):
    return not np.array_equal(a["X"], b["X"])


# ---------------------------------------------------------------------------------------------------------------------
# 1. an updated handle is a fresh handle on the new matrices
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,dtype", [(k, "f64") for k in mc.UNSCALED] + [(mc.CACHED, "f32"), (mc.RANDOM, "f32")], ids=str)
def test_updated_handle_equals_a_fresh_handle_on_the_new_matrices(gpu, key, dtype):
    kw = mc.solve_kw(key)
    with make(gpu, key, 0, 0, dtype) as h:
        first = run(h, **kw)
        h.update_matrices(*mc.matrices(key, 1))
        second = run(h, **kw)                                              # cold, from X = 0 as the fresh handle
    want = fresh(gpu, key, 1, 1, dtype)
    print(key, dtype, "iterations", [i["iterations"] for i in second["infos"]][:8], "resPrim", second["infos"][0]["resPrim"], want["infos"][0]["resPrim"])
    assert same(second, want)
    assert differ(first, second)                                           # the matrices did change the problem
    if mc.to_tolerance(key) and dtype == "f64":                            # (an fp32 handle does not reach 1e-6 on these families; its identity holds all the same)
        assert max(i["iterations"] for i in second["infos"]) < mc.NUM_ITERATIONS


# ---------------------------------------------------------------------------------------------------------------------
# 2. partial updates
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ONE_PER_KIND, ids=str)
def test_partial_updates_equal_fresh_handles_and_an_empty_update_changes_nothing(gpu, key):
    kw = mc.solve_kw(key)
    P2, A2 = mc.matrices(key, 1)
    with make(gpu, key) as h:
        run(h, **kw)
        h.update_matrices(mP=P2)
        p_only = run(h, **kw)
        assert same(p_only, fresh(gpu, key, 1, 0))
        h.update_matrices()                                                # both NULL: QPS_OK, nothing changes, the factor stays valid
        again = run(h, reuseFactor=True, **kw)
        assert same(again, p_only)
    with make(gpu, key) as h:
        run(h, **kw)
        h.update_matrices(mA=A2)
        assert same(run(h, **kw), fresh(gpu, key, 0, 1))
    assert differ(fresh(gpu, key, 1, 0), fresh(gpu, key, 0, 1))


# ---------------------------------------------------------------------------------------------------------------------
# 3. round trip
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ONE_PER_KIND + [mc.LASSO], ids=str)
def test_round_trip_returns_to_the_first_solve(gpu, key):
    kw = mc.solve_kw(key)
    with make(gpu, key) as h:
        first = run(h, **kw)
        h.update_matrices(*mc.matrices(key, 1))
        middle = run(h, **kw)
        h.update_matrices(*mc.matrices(key, 0))
        last = run(h, **kw)
    assert differ(first, middle)
    assert same(last, first)


# ---------------------------------------------------------------------------------------------------------------------
# 4. options and state are carried across the update
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ONE_PER_KIND, ids=str)
def test_options_and_state_are_carried(gpu, key):
    """Per-row rho scale, family-wide rho rule and warm start "state" on (the CG handle has all three; it lacks the equilibration alone, which is test 5)."""
    _, _, Q, L, U = mc.data(key)
    kw = mc.solve_kw(key)
    vS = gpu.equality_rho_scale(L, U, 1e2)
    vS[0] = 10.0                                                           # a scale that is not all ones on any family

    def options(h):
        h.set_rho_scale(vS)
        h.set_adaptive_rho(True)
        h.set_warm_start("state")

    results = []
    for reuse in (False, True):
        with make(gpu, key) as h:
            options(h)
            r1 = run(h, **kw)
            h.update_matrices(*mc.matrices(key, 1))
            results.append((r1, run(h, r1["X"], reuseFactor=reuse, **kw)))
    (r1, r2), (r1b, r2b) = results
    assert same(r1, r1b)
    with make(gpu, key, 1, 1) as twin:
        options(twin)
        twin.set_dual(r1["Z"], r1["Y"])
        want = run(twin, r1["X"], **kw)
    with make(gpu, key, 1, 1) as cold:                                     # the state matters: the same handle without it ends elsewhere
        options(cold)
        assert not same(run(cold, r1["X"], **kw), want)
    print(key, "iterations after the update", [i["iterations"] for i in r2["infos"]][:8], "numRefactor", [i["numRefactor"] for i in r2["infos"]][:8])
    assert same(r2, want)
    assert same(r2b, want)                                                 # reuseFactor on the first solve after an update still factorises


# ---------------------------------------------------------------------------------------------------------------------
# 5. equilibration on: the exponents are kept, exactly
# ---------------------------------------------------------------------------------------------------------------------
def scaled_twin_data(key, D, E, k=1):
    """(D P_k D, E A_k D, D q, E l, E u): exact, D and E are powers of two."""
    _, _, Q, L, U = mc.data(key)
    P2, A2 = mc.matrices(key, k)
    if sp.issparse(P2):
        Pc, Ac = mc.canonical(P2), mc.canonical(A2)
        n = Pc.shape[0]
        pcol, acol = np.repeat(np.arange(n), np.diff(Pc.indptr)), np.repeat(np.arange(n), np.diff(Ac.indptr))
        Pt = sp.csc_matrix((Pc.data * (D[Pc.indices] * D[pcol]), Pc.indices.copy(), Pc.indptr.copy()), shape=Pc.shape)
        At = sp.csc_matrix((Ac.data * (E[Ac.indices] * D[acol]), Ac.indices.copy(), Ac.indptr.copy()), shape=Ac.shape)
    else:
        Pt, At = D[:, None] * P2 * D[None, :], E[:, None] * A2 * D[None, :]
    return Pt, At, Q * D, L * E, U * E


@pytest.mark.parametrize("key", [mc.SCRAMBLED, mc.SCRAMBLED_SPARSE], ids=str)
def test_kept_exponents_are_exact(gpu, key):
    kw = mc.solve_kw(key)
    assert not mc.to_tolerance(key)                                        # eps = 0, a fixed iteration count: the twin stops where the handle stops
    cls = getattr(gpu, CLASSES[mc.kind_of(key)])
    with make(gpu, key) as h:
        h.set_equilibration(mc.PASSES)
        D, E = h.equilibration()
        assert (D != 1).any() and (E != 1).any()
        run(h, **kw)
        h.update_matrices(*mc.matrices(key, 1))
        D2, E2 = h.equilibration()
        assert np.array_equal(D, D2) and np.array_equal(E, E2)
        r = run(h, **kw)                                                   # X = 0
        with cls(*scaled_twin_data(key, D, E)) as twin:
            t = run(twin, **kw)
        assert np.array_equal(r["X"], D * t["X"]) and np.array_equal(r["Y"], E * t["Y"]) and np.array_equal(r["Z"], t["Z"] / E)
        assert r["flags"] == t["flags"] and [i["iterations"] for i in r["infos"]] == [i["iterations"] for i in t["infos"]]
        h.set_equilibration(mc.PASSES)                                     # a scaling computed from the new matrices
        again = run(h, **kw)
        Dn, En = h.equilibration()
    with make(gpu, key, 1, 1) as f:
        f.set_equilibration(mc.PASSES)
        Df, Ef = f.equilibration()
        want = run(f, **kw)
    assert np.array_equal(Dn, Df) and np.array_equal(En, Ef)
    assert same(again, want)


OTHER_PASSES = 3                                                           # a second scaling: on these matrices its exponents are not those of mc.PASSES


def test_a_change_of_scaling_between_two_updates(gpu):
    """Sparse L D L' handle: scaling of mc.PASSES passes, update to step 1, scaling of OTHER_PASSES passes, update to step 2, scaling off, update to step 3; a
    solve of mc.FIXED_ITERATIONS iterations at every stop.  The per-entry exponents of the update are built under the first scaling, dropped and rebuilt under
    the second, and gone with the third.

    An update keeps the exponents of the matrices it found, and those are not the exponents a fresh handle computes from the new matrices (on these families
    they differ at every step and every pass count).  So the fresh handle "on those matrices with the same options" is: right after an update under a scaling,
    the unscaled twin on (D P_k D, E A_k D) of test 5 -- X, Y, Z exact through D and E, flags and iteration counts equal, D and E unchanged by the update; after
    every change of scaling and after the unscaled update, a fresh handle with that pass count -- ``same()``: X, Z, Y and every qps_info field but the times --
    and its exponent vectors."""
    key = mc.SCRAMBLED_SPARSE
    kw = dict(numIterations=mc.FIXED_ITERATIONS, ϵAbs=0.0, ϵRel=0.0, ρ=mc.rho_of(key))

    def fresh_with(k, passes):
        with make(gpu, key, k, k) as f:
            f.set_equilibration(passes)
            return run(f, **kw), f.equilibration()

    def update_under_kept_exponents(h, k):
        D, E = h.equilibration()
        assert (D != 1).any() and (E != 1).any()
        h.update_matrices(*mc.matrices(key, k))
        assert all(np.array_equal(a, b) for a, b in zip(h.equilibration(), (D, E)))
        r = run(h, **kw)
        with gpu.QuadraticProgramSparseSharedBatch(*scaled_twin_data(key, D, E, k)) as twin:
            t = run(twin, **kw)
        assert np.array_equal(r["X"], D * t["X"]) and np.array_equal(r["Y"], E * t["Y"]) and np.array_equal(r["Z"], t["Z"] / E), k
        assert r["flags"] == t["flags"] and [i["iterations"] for i in r["infos"]] == [i["iterations"] for i in t["infos"]]

    def equals_fresh(h, k, passes):
        want, (Df, Ef) = fresh_with(k, passes)
        D, E = h.equilibration()
        assert np.array_equal(D, Df) and np.array_equal(E, Ef), (k, passes)
        assert same(run(h, **kw), want), (k, passes)
        return D, E

    with make(gpu, key) as h:
        h.set_equilibration(mc.PASSES)
        update_under_kept_exponents(h, 1)
        D1, E1 = h.equilibration()
        h.set_equilibration(OTHER_PASSES)
        D2, E2 = equals_fresh(h, 1, OTHER_PASSES)
        assert not (np.array_equal(D1, D2) and np.array_equal(E1, E2))    # the scaling did change between the two updates
        update_under_kept_exponents(h, 2)
        h.set_equilibration(0)
        equals_fresh(h, 2, 0)
        h.update_matrices(*mc.matrices(key, 3))
        equals_fresh(h, 3, 0)


def test_three_updates_in_a_row_on_a_cg_handle(gpu):
    """The unscaled part of the sequence above on the CG handle, which refuses the equilibration: after each of three updates a solve of mc.FIXED_ITERATIONS
    iterations equals a fresh handle's on those matrices."""
    key = mc.CG_BANDED
    kw = dict(numIterations=mc.FIXED_ITERATIONS, ϵAbs=0.0, ϵRel=0.0, ρ=mc.rho_of(key))
    with make(gpu, key) as h:
        for k in (1, 2, 3):
            h.update_matrices(*mc.matrices(key, k))
            got = run(h, **kw)
            with make(gpu, key, k, k) as f:
                assert same(got, run(f, **kw)), k



# ---------------------------------------------------------------------------------------------------------------------
# 6. polishing and certificates
# ---------------------------------------------------------------------------------------------------------------------
def _polish_pair(gpu, cls, P, A, Q, L, U, rho):
    P2, A2 = mc.step_matrices(P, A, 1)
    kw = dict(numIterations=mc.NUM_ITERATIONS, ϵAbs=1e-6, ϵRel=1e-6, ρ=rho)
    out = []
    for updated in (True, False):
        with (cls(P, A, Q, L, U) if updated else cls(P2, A2, Q, L, U)) as h:
            if updated:
                run(h, **kw)
                h.update_matrices(P2, A2)
            r = run(h, **kw)
            X = r["X"].copy()
            reps = h.polish(X)                                             # y: what the handle holds
            out.append((r, X, [{k: v for k, v in rep.items() if k != "seconds"} for rep in reps]))
    return out


@pytest.mark.parametrize("kind", ["cg", "dense"])
def test_polish_on_an_updated_handle_equals_a_fresh_handle(gpu, kind):
    if kind == "cg":
        (ru, Xu, repu), (rf, Xf, repf) = _polish_pair(gpu, gpu.QuadraticProgramCgSharedBatch, *cc.polish_family(cc.COUNT), cc.RHO["banded"])
    else:
        (ru, Xu, repu), (rf, Xf, repf) = _polish_pair(gpu, gpu.QuadraticProgramSharedBatch, *mc.data(mc.CACHED), mc.RHO)
    print(kind, "polish flags", [r["flag"] for r in repu], "refinements", [r["refinements"] for r in repu])
    assert same(ru, rf)
    assert np.array_equal(Xu, Xf) and repr(repu) == repr(repf)
    if kind == "cg":                                                       # polish_family is built so that the step succeeds
        assert any(r["flag"] == 0 for r in repu) and not np.array_equal(Xu, ru["X"])


def test_certificate_is_zero_between_an_update_and_the_next_solve(gpu):
    name = "dense-primal-r1"
    P, A, Q, L, U = ic.case_data(name)
    with gpu.QuadraticProgramSharedBatch(P, A, Q, L, U) as h:
        h.set_infeasibility(1e-4, 1e-4)
        _, flags, _ = h.solve(numIterations=5000, ϵAbs=1e-6, ϵRel=1e-6, ρ=1.0)
        assert [int(f) for f in flags] == ic.CASES[name]["flags"] and 4 in [int(f) for f in flags]
        DY, DX = h.certificate()
        assert DY.any()
        h.update_matrices(mP=mc.step_matrices(P, A, 1)[0])
        DY, DX = h.certificate()
        assert not DY.any() and not DX.any()
        _, flags, _ = h.solve(numIterations=5000, ϵAbs=1e-6, ϵRel=1e-6, ρ=1.0)          # the rows of A did not move: the same column has no solution
        assert int(flags[4]) == 4 and h.certificate()[0][4].any()


# ---------------------------------------------------------------------------------------------------------------------
# 7. refusals leave the handle bit for bit what it was
# ---------------------------------------------------------------------------------------------------------------------
def _csc_args(M):
    c = mc.canonical(M)
    return c.indptr.astype(np.int64), c.indices.astype(np.int64), np.ascontiguousarray(c.data, dtype=np.float64)


def _ip(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int64))


def _dp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def _raw_csc(h, P=(None, None, None), A=(None, None, None), base=0):
    from quadraticprogramsolver_amd import _lib
    L = _lib.lib()
    rc = L.qps_update_shared_matrices_csc(h._h, _ip(P[0]), _ip(P[1]), _dp(P[2]), _ip(A[0]), _ip(A[1]), _dp(A[2]), base)
    return rc, L.qps_last_error(h._h).decode()


def _raw_dense(h, P=None, A=None):
    from quadraticprogramsolver_amd import _lib
    L = _lib.lib()
    Pf, Af = (None if M is None else np.asfortranarray(M, dtype=np.float64) for M in (P, A))
    rc = L.qps_update_shared_matrices(h._h, _dp(Pf), h.n, _dp(Af), h.m)
    return rc, L.qps_last_error(h._h).decode()


def _pattern_variants(M):
    """(name, (colptr, rowval, nzval)) of three matrices near M's pattern: one row index moved within a column, one entry more, one entry fewer."""
    cp, ri, nz = _csc_args(M)
    rows = M.shape[0]
    j = next(j for j in range(len(cp) - 1) if 0 < cp[j + 1] - cp[j] < rows)          # a column with a free row
    taken = set(ri[cp[j]:cp[j + 1]].tolist())
    free = next(r for r in range(rows) if r not in taken)
    moved = ri.copy()
    moved[cp[j]] = free
    order = np.argsort(moved[cp[j]:cp[j + 1]], kind="stable")
    moved_nz = nz.copy()
    moved[cp[j]:cp[j + 1]], moved_nz[cp[j]:cp[j + 1]] = moved[cp[j]:cp[j + 1]][order], nz[cp[j]:cp[j + 1]][order]
    more_cp = cp.copy()
    more_cp[j + 1:] += 1
    at = cp[j] + int(np.searchsorted(ri[cp[j]:cp[j + 1]], free))
    more = (more_cp, np.insert(ri, at, free), np.insert(nz, at, 0.5))
    fewer_cp = cp.copy()
    fewer_cp[j + 1:] -= 1
    fewer = (fewer_cp, np.delete(ri, cp[j]), np.delete(nz, cp[j]))
    return j, [("moved", (cp, moved, moved_nz)), ("more", more), ("fewer", fewer)]


@pytest.mark.parametrize("key", [mc.RANDOM, mc.CG_BANDED], ids=str)
def test_refusals_of_the_csc_entry_point_leave_the_handle_untouched(gpu, key):
    kw = mc.solve_kw(key)
    P0, A0 = mc.matrices(key, 0)
    P2, A2 = mc.matrices(key, 1)
    with make(gpu, key) as h:
        before = run(h, **kw)

        def refused(what, rc, msg, code, text):
            print(f"{key} {what}: {rc} {msg}")
            assert rc == code and text in msg, (what, rc, msg)
            assert same(run(h, reuseFactor=True, **kw), before), what

        rc, msg = _raw_dense(h, ec._dense(P2), None)
        refused("dense entry point", rc, msg, UNSUPPORTED, "qps_update_shared_matrices_csc")
        cp, ri, nz = _csc_args(P2)
        asym = nz.copy()
        k = next(k for j in range(len(cp) - 1) for k in range(cp[j], cp[j + 1]) if ri[k] != j)          # an off-diagonal entry
        asym[k] *= 1.5
        rc, msg = _raw_csc(h, P=(cp, ri, asym))
        refused("asymmetric P", rc, msg, BAD_ARGUMENT, "The matrix mP must be a symmetric positive definite matrix (asymmetric entry in column")
        acp, ari, anz = _csc_args(A2)
        nan = anz.copy()
        nan[len(nan) // 2] = np.nan
        rc, msg = _raw_csc(h, P=(cp, ri, nz), A=(acp, ari, nan))           # a good P beside it must not get in
        refused("NaN in A", rc, msg, NOT_FINITE, "A contains NaN/Inf")
        j, variants = _pattern_variants(A2)
        for what, arrays in variants:
            rc, msg = _raw_csc(h, P=(cp, ri, nz), A=arrays)
            refused(f"A pattern: {what}", rc, msg, BAD_ARGUMENT, f"pattern of A differs from the handle's (first in column {j},")
        rc, msg = _raw_csc(h, P=(cp, None, nz))
        refused("two of three pointers", rc, msg, BAD_ARGUMENT, "of P must be all NULL")
        rc, msg = _raw_csc(h, A=(acp, ari, None))
        refused("two of three pointers", rc, msg, BAD_ARGUMENT, "of A must be all NULL")
        # an explicit zero is part of the pattern: A with one stored entry set to zero is accepted, the same entry eliminated is not
        zeroed = anz.copy()
        zeroed[0] = 0.0
        Az = sp.csc_matrix((zeroed, ari.copy(), acp.copy()), shape=A2.shape)
        Ae = Az.copy()
        Ae.eliminate_zeros()
        rc, msg = _raw_csc(h, A=_csc_args(Ae))
        refused("eliminated zero", rc, msg, BAD_ARGUMENT, "pattern of A differs")
        h.update_matrices(mA=Az)
        h.update_matrices(P0, A0)
        assert same(run(h, **kw), before)


def test_refusals_of_the_dense_entry_point_leave_the_handle_untouched(gpu):
    key = mc.CACHED
    kw = mc.solve_kw(key)
    P2, A2 = mc.matrices(key, 1)
    with make(gpu, key) as h:
        before = run(h, **kw)

        def refused(what, rc, msg, code, text):
            print(f"{what}: {rc} {msg}")
            assert rc == code and text in msg, (what, rc, msg)
            assert same(run(h, reuseFactor=True, **kw), before), what

        rc, msg = _raw_csc(h, P=_csc_args(sp.csc_matrix(P2)))
        refused("CSC entry point", rc, msg, UNSUPPORTED, "qps_update_shared_matrices")
        asym = P2.copy()
        asym[3, 7] += 1e-3
        rc, msg = _raw_dense(h, asym, A2)
        refused("asymmetric P", rc, msg, BAD_ARGUMENT, "The matrix mP must be a symmetric positive definite matrix (asymmetric entry in column 3)")
        nan = A2.copy()
        nan[5, 5] = np.nan
        rc, msg = _raw_dense(h, P2, nan)
        refused("NaN in A", rc, msg, NOT_FINITE, "A contains NaN/Inf")
        inf = P2.copy()
        inf[2, 2] = np.inf
        rc, msg = _raw_dense(h, inf, None)
        refused("Inf in P", rc, msg, NOT_FINITE, "P contains NaN/Inf")
        with pytest.raises(ValueError, match="dimension mismatch"):
            h.update_matrices(mP=P2[:-1, :-1])


def test_a_stand_alone_handle_is_refused_by_both_entry_points(gpu):
    P, A, Q, L, U = mc.data(mc.CACHED)
    with gpu.QuadraticProgram(P, Q[0], A, L[0], U[0]) as h:
        x0 = np.zeros(h.n)
        f0 = h.solve(x0, numIterations=200, ρ=mc.RHO)
        from quadraticprogramsolver_amd import _lib
        Lb = _lib.lib()
        Pf = np.asfortranarray(P)
        rc = Lb.qps_update_shared_matrices(h._h, _dp(Pf), P.shape[0], None, 0)
        msg = Lb.qps_last_error(h._h).decode()
        assert rc == UNSUPPORTED and "only shared-matrix batch handles" in msg, (rc, msg)
        cp, ri, nz = _csc_args(sp.csc_matrix(P))
        rc = Lb.qps_update_shared_matrices_csc(h._h, _ip(cp), _ip(ri), _dp(nz), None, None, None, 0)
        msg = Lb.qps_last_error(h._h).decode()
        assert rc == UNSUPPORTED and "only shared-matrix batch handles" in msg, (rc, msg)
        x1 = np.zeros(h.n)
        f1 = h.solve(x1, numIterations=200, ρ=mc.RHO)
        assert np.array_equal(x0, x1) and f0 == f1 and x0.any()


@pytest.mark.parametrize("kind", ["dense", "sparse"])
def test_the_fp32_range_case_is_refused_under_the_kept_exponents(gpu, kind):
    P, A1, A2, Q, L, U = mc.range_case()
    cls = getattr(gpu, CLASSES[kind])
    wrap = (lambda M: M) if kind == "dense" else sp.csc_matrix
    kw = dict(numIterations=50, ϵAbs=0.0, ϵRel=0.0, ρ=mc.RHO)
    with cls(wrap(P), wrap(A1), Q, L, U, dtype="f32") as h:
        h.set_equilibration(mc.PASSES)
        D, E = h.equilibration()
        before = run(h, **kw)
        from quadraticprogramsolver_amd._lib import QpsError
        with pytest.raises(QpsError) as err:
            h.update_matrices(mA=wrap(A2))
        print(kind, err.value)
        assert err.value.status == UNSUPPORTED and "would leave the normal range" in err.value.message and "the handle is unchanged" in err.value.message
        D2, E2 = h.equilibration()
        assert np.array_equal(D, D2) and np.array_equal(E, E2)
        assert same(run(h, reuseFactor=True, **kw), before)
    with cls(wrap(P), wrap(A1), Q, L, U, dtype="f64") as h:               # the same update on an fp64 handle is in range
        h.set_equilibration(mc.PASSES)
        h.update_matrices(mA=wrap(A2))
