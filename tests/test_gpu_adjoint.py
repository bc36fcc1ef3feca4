"""The adjoint derivatives on the shared-matrix batches on the device (qps_adjoint_shared) through the Python binding, against the direct reference of
tests/adjoint_cases.py (tests/test_adjoint_cpu.py guards it).  Both sides get the same x, y and g_x.  Every bound is 4 x the distance of the numpy restatement of
the refinement rounds from that reference, measured on a CPU and recorded in adjoint_cases.BOUNDS; every figure is printed before it is asserted."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import adjoint_cases as cases

pytestmark = pytest.mark.gpu

BAD_ARGUMENT, UNSUPPORTED = 1, 8
PARITY = cases.PARITY
VECTORS, VALUES = ("dQ", "dL", "dU"), ("vP", "vA")
REPORT_KEYS = ("flag", "refinements", "minresIterations", "numActiveLower", "numActiveUpper", "relres")


def handle(gpu, kind, data, **kw):
    P, A, Q, L, U = data
    if kind == "dense":
        return gpu.QuadraticProgramSharedBatch(P, A, Q, L, U, **kw)
    cls = gpu.QuadraticProgramSparseSharedBatch if kind == "sparse" else gpu.QuadraticProgramCgSharedBatch
    return cls(sp.csc_matrix(P), sp.csc_matrix(A), Q, L, U, **kw)


def check(key, out, ref, keys):
    """Prints the distance of every output in ``keys`` from the reference (per column for the vectors), then asserts the recorded bound."""
    worst = {}
    for k in keys:
        worst[k] = cases.distance(out[k], ref[k])
        print(f"{key} {k}: distance {worst[k]:.2e} (restatement {cases.BOUNDS[key][k]:.2e}, bound {cases.bound(key, k):.2e})")
    for k in keys:
        assert worst[k] <= cases.bound(key, k), (key, k)


def check_pattern(prob, ref):
    assert all(np.array_equal(a, b) for a, b in zip(prob.pattern(), ref["pattern"]))


def run(gpu, kind, name, count, settings=PARITY, **kw):
    data, X, Y = cases.case(name, count)
    with handle(gpu, kind, data, **kw) as prob:
        out = prob.adjoint(cases.GX(count, X.shape[1]), X, Y, **settings)
        if kind != "dense":
            check_pattern(prob, cases.reference(name, count))
    for b in range(count):
        assert out["reports"][b]["numActiveLower"] == int((Y[b] < 0).sum()) and out["reports"][b]["numActiveUpper"] == int((Y[b] > 0).sum())
    print(f"{kind} {name} count {count}: flags {[r['flag'] for r in out['reports']]} MINRES {[r['minresIterations'] for r in out['reports']]}")
    return out


@pytest.mark.parametrize("count", [3, 20, 37])
def test_dense_parity_in_every_panel_geometry(gpu, count):
    """One panel, two panels with a ragged second, three panels: 13, 12 and 11 padding columns."""
    out = run(gpu, "dense", "dense", count)
    assert all(r["flag"] == 0 for r in out["reports"]) and out["vP"] is None and out["vA"] is None
    check(f"dense-{count}", out, cases.reference("dense", count), VECTORS)


@pytest.mark.parametrize("kind", ["sparse", "cg"])
@pytest.mark.parametrize("count", [3, 20])
def test_sparse_and_cg_parity_with_value_gradients(gpu, kind, count):
    out = run(gpu, kind, "random", count)
    assert all(r["flag"] == 0 for r in out["reports"])
    check(f"random-{count}", out, cases.reference("random", count), VECTORS + VALUES)


@pytest.mark.parametrize("name", ["banded", "banded71", "banded_long"])
def test_entry_counts_and_the_grid_stride(gpu, name):
    """banded_family(3) at n = 70 has 208 = 13 x 16 stored entries in each of P and A: whole rows of a workgroup.  n = 71 has 211 and n = LONG_N 98998: no multiple
    of a wave's four rows of lanes, of a workgroup's 16 rows nor of its 64 entries per trip, and the latter is more than one sweep of the capped grid (1024
    workgroups of 64 entries)."""
    ref = cases.reference(name, 3)
    nP, nA = ref["pattern"][1].size, ref["pattern"][3].size
    print(f"{name}: nnz(P) {nP} nnz(A) {nA}")
    assert name == "banded" or (nP % 4 and nA % 4 and nP % 16 and nA % 16 and nP % 64 and nA % 64)
    assert name != "banded_long" or min(nP, nA) > 1024 * 64
    out = run(gpu, "cg", name, 3)
    assert all(r["flag"] == 0 for r in out["reports"])
    check(f"{name}-3", out, ref, VECTORS + VALUES)


def test_bit_identities(gpu):
    """Two runs agree in every bit; a column of the batch of 20 equals the batch of one in dQ, dL, dU; with g_x zero in all columns but one the value gradients
    equal those of the batch of one; a solve after the call is the solve without it."""
    data, X, Y = cases.case("random", 20)
    P, A, Q, L, U = data
    G = cases.GX(20, X.shape[1])
    kw = dict(ρ=0.1, ϵAbs=1e-4, ϵRel=1e-4)
    with handle(gpu, "sparse", data) as prob:
        X0, f0, i0 = prob.solve(**kw)
        Z0, Y0 = prob.dual()
    with handle(gpu, "sparse", data) as prob:
        o1 = prob.adjoint(G, X, Y, **PARITY)
        o2 = prob.adjoint(G, X, Y, **PARITY)
        G17 = np.zeros_like(G); G17[17] = G[17]
        o17 = prob.adjoint(G17, X, Y, **PARITY)
        X1, f1, i1 = prob.solve(**kw)
        Z1, Y1 = prob.dual()
    for k in VECTORS + VALUES:
        assert np.array_equal(o1[k], o2[k]) and o1[k].any(), k
    assert [[r[k] for k in REPORT_KEYS] for r in o1["reports"]] == [[r[k] for k in REPORT_KEYS] for r in o2["reports"]]
    assert np.array_equal(X1, X0) and np.array_equal(Z1, Z0) and np.array_equal(Y1, Y0) and list(f1) == list(f0)
    assert [[i[k] for k in ("iterations", "resPrim", "resDual")] for i in i1] == [[i[k] for k in ("iterations", "resPrim", "resDual")] for i in i0]
    for b in (0, 16, 17, 19):
        with handle(gpu, "sparse", (P, A, Q[b:b + 1], L[b:b + 1], U[b:b + 1])) as one:
            o = one.adjoint(G[b:b + 1], X[b:b + 1], Y[b:b + 1], **PARITY)
        for k in VECTORS:
            assert np.array_equal(o[k][0], o1[k][b]), (k, b)
        assert [o["reports"][0][k] for k in REPORT_KEYS] == [o1["reports"][b][k] for k in REPORT_KEYS], b
        if b == 17:
            assert np.array_equal(o["vP"], o17["vP"]) and np.array_equal(o["vA"], o17["vA"]) and o["vP"].any() and o["vA"].any()
            assert not np.delete(o17["dQ"], 17, axis=0).any()


def test_exact_zeros(gpu):
    """y = 0: dL, dU and vA are exactly zero.  A column with g_x = 0 has a zero row and contributes nothing to the sums."""
    data, X, Y = cases.case("random", 3)
    G = cases.GX(3, X.shape[1])
    ref = cases.reference("random", 3)
    with handle(gpu, "sparse", data) as prob:
        o = prob.adjoint(G, X, np.zeros_like(Y), **PARITY)
        G1 = G.copy(); G1[1] = 0.0
        o1 = prob.adjoint(G1, X, Y, **PARITY)
    assert all(r["flag"] == 0 and r["numActiveLower"] == 0 and r["numActiveUpper"] == 0 for r in o["reports"])
    assert not o["dL"].any() and not o["dU"].any() and not o["vA"].any() and o["dQ"].any() and o["vP"].any()
    check("random_zero_y-3", o, cases.reference("random_zero_y", 3), ("dQ", "vP"))
    assert o1["reports"][1]["flag"] == 0 and o1["reports"][1]["minresIterations"] == 0
    assert not o1["dQ"][1].any() and not o1["dL"][1].any() and not o1["dU"][1].any()
    check("random-3", o1, cases.flag_reference(ref, (1,)), VECTORS + VALUES)


def test_flags_are_per_column(gpu):
    """numItrPolish = 1 under a MINRES cap that the columns of FLAG_COLUMNS_OVER exceed (tests/test_adjoint_cpu.py): zero rows, flag 1, absent from vP and vA."""
    name, count = cases.FLAG_CASE
    out = run(gpu, "sparse", name, count, dict(PARITY, numItrPolish=1, numItrMinres=cases.FLAG_CAP))
    for b in range(count):
        r = out["reports"][b]
        if b in cases.FLAG_COLUMNS_OVER:
            assert r["flag"] == 1 and r["refinements"] == 1 and r["minresIterations"] == cases.FLAG_CAP, b
            assert not out["dQ"][b].any() and not out["dL"][b].any() and not out["dU"][b].any(), b
        else:
            assert r["flag"] == 0 and out["dQ"][b].any(), b
    check(f"{name}-{count}-flag", out, cases.flag_reference(cases.reference(name, count), cases.FLAG_COLUMNS_OVER), VECTORS + VALUES)


@pytest.mark.parametrize("kind,name", [("dense", "scrambled"), ("sparse", "scrambled_random")])
def test_equilibration_results_are_in_the_callers_units(gpu, kind, name):
    data, X, Y = cases.case(name, 4)
    D, E = cases.equilibration_of(name)
    with handle(gpu, kind, data) as prob:
        prob.set_equilibration(cases.EQUIL_PASSES)
        d, e = prob.equilibration()
        out = prob.adjoint(cases.GX(4, X.shape[1]), X, Y, **PARITY)
    assert np.array_equal(d, D) and np.array_equal(e, E) and (D != 1).any() and (E != 1).any()
    print(f"{name}: flags {[r['flag'] for r in out['reports']]} MINRES {[r['minresIterations'] for r in out['reports']]}")
    assert all(r["flag"] == 0 for r in out["reports"])
    check(f"{name}-4-equilibrated", out, cases.reference(name, 4), VECTORS + (VALUES if kind == "sparse" else ()))


@pytest.mark.parametrize("kind,name", [("dense", "dense"), ("sparse", "random")])
def test_fp32_handles(gpu, kind, name):
    out = run(gpu, kind, name, 3, cases.FP32, dtype="f32")
    assert all(r["flag"] == 0 for r in out["reports"])
    check(f"{name}-3-fp32", out, cases.reference(name, 3), VECTORS + (VALUES if kind == "sparse" else ()))


@pytest.mark.parametrize("kind,name,equilibrate", [("dense", "dense", False), ("sparse", "random", True)])
def test_no_y_takes_the_y_of_the_handle(gpu, kind, name, equilibrate):
    data, _, _ = cases.case(name, 20)
    G = cases.GX(20, data[0].shape[0])
    settings = dict(PARITY, numItrPolish=2, numItrMinres=200)
    with handle(gpu, kind, data) as prob:
        if equilibrate:
            prob.set_equilibration(cases.EQUIL_PASSES)
        X, _, _ = prob.solve(ρ=0.1, ϵAbs=1e-4, ϵRel=1e-4)
        Y = prob.dual()[1]
        o1 = prob.adjoint(G, X, None, **settings)
        o2 = prob.adjoint(G, X, Y, **settings)
    assert Y.any()
    for k in VECTORS + (VALUES if kind == "sparse" else ()):
        assert np.array_equal(o1[k], o2[k]), k
    assert [[r[k] for k in REPORT_KEYS] for r in o1["reports"]] == [[r[k] for k in REPORT_KEYS] for r in o2["reports"]]
    assert any(r["numActiveLower"] + r["numActiveUpper"] > 0 for r in o1["reports"])


def test_refusals(gpu):
    from quadraticprogramsolver_amd import _lib
    L_ = _lib.lib()
    (P, A, Q, L, U), X, Y = cases.case("dense", 3)
    G = cases.GX(3, X.shape[1])
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    p = _lib.default_params()
    dq = np.zeros_like(X)
    with gpu.QuadraticProgram(P, Q[0], A, L[0], U[0]) as one, gpu.QuadraticProgramBatch([(P, Q[b], A, L[b], U[b]) for b in range(2)]) as batch:
        for h in (one._h, batch._h):
            assert L_.qps_adjoint_shared(h, ptr(X), ptr(Y), ptr(G), C.byref(p), ptr(dq), None, None, None, None, None) == UNSUPPORTED
            assert b"shared-matrix batch" in L_.qps_last_error(h)
    assert not dq.any()
    with handle(gpu, "dense", (P, A, Q, L, U)) as prob:
        for bad_x, bad_y, bad_g in ((True, False, False), (False, True, False), (False, False, True)):
            for v in (np.nan, np.inf):
                x, y, g = X.copy(), Y.copy(), G.copy()
                (x if bad_x else y if bad_y else g)[2, 3] = v
                with pytest.raises(gpu.QpsError) as e:
                    prob.adjoint(g, x, y, **PARITY)
                assert e.value.status == BAD_ARGUMENT
        for kw in (dict(δ=np.inf), dict(δ=np.nan), dict(ϵMinres=np.nan)):
            with pytest.raises(gpu.QpsError) as e:
                prob.adjoint(G, X, Y, **kw)
            assert e.value.status == BAD_ARGUMENT
        assert L_.qps_adjoint_shared(prob._h, None, ptr(Y), ptr(G), C.byref(p), ptr(dq), None, None, None, None, None) == BAD_ARGUMENT
        assert L_.qps_adjoint_shared(prob._h, ptr(X), ptr(Y), None, C.byref(p), ptr(dq), None, None, None, None, None) == BAD_ARGUMENT
        assert L_.qps_adjoint_shared(prob._h, ptr(X), ptr(Y), ptr(G), None, ptr(dq), None, None, None, None, None) == BAD_ARGUMENT
        v = np.zeros(P.size)
        assert L_.qps_adjoint_shared(prob._h, ptr(X), ptr(Y), ptr(G), C.byref(p), ptr(dq), None, None, ptr(v), None, None) == UNSUPPORTED
        assert L_.qps_adjoint_shared(prob._h, ptr(X), ptr(Y), ptr(G), C.byref(p), ptr(dq), None, None, None, ptr(v), None) == UNSUPPORTED
        assert b"dense shared-matrix batch" in L_.qps_last_error(prob._h) and not dq.any() and not v.any()
        with pytest.raises(ValueError):
            prob.adjoint(G[:2], X, Y)
        out = prob.adjoint(G, X, Y, **PARITY)                                 # the handle stays usable
        assert all(r["flag"] == 0 for r in out["reports"])
        check("dense-3", out, cases.reference("dense", 3), VECTORS)
        out = prob.adjoint(G, X, Y, numItrPolish=0)                           # the rounds never ran: flag -1, zeros
        assert all(r["flag"] == -1 and r["refinements"] == 0 for r in out["reports"]) and not out["dQ"].any() and not out["dL"].any()
    data, Xr, Yr = cases.case("random", 3)
    with handle(gpu, "sparse", data) as prob:
        out = prob.adjoint(cases.GX(3, Xr.shape[1]), Xr, Yr, matrices=False, **PARITY)
        assert out["vP"] is None and out["vA"] is None
        check("random-3", out, cases.reference("random", 3), VECTORS)
