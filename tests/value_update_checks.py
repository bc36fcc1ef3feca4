"""The device checks of qps_update_shared_values that run once per input location: from numpy arrays inside the pytest process
(tests/test_gpu_value_update.py) and from torch device tensors in a child process that imports torch before the library, so that the process holds one HIP
runtime (tests/value_update_device_child.py).  ``wrap`` turns a float64 numpy vector into what ``update_values`` is given.  Every check raises AssertionError.
The reference is the library itself: a twin handle that takes the same values through ``update_matrices``; ``same()`` of tests/test_gpu_warm_start.py compares
X, Z, Y, flags and every qps_info field but the wall times, bit for bit."""
import numpy as np
import scipy.sparse as sp

import matrix_update_cases as mc
import value_update_cases as vc
from test_gpu_warm_start import run, same

BAD_ARGUMENT, NOT_FINITE, UNSUPPORTED = 1, 3, 8


def make(gpu, key, dtype="f64", P=None):
    P0, A0, Q, L, U = mc.data(key)
    return getattr(gpu, vc.CLASSES[mc.kind_of(key)])(P0 if P is None else P, A0, Q, L, U, dtype=dtype)


def refusal(call):
    from quadraticprogramsolver_amd._lib import QpsError
    try:
        call()
    except QpsError as e:
        return e.status, e.message
    raise AssertionError("the call was not refused")


def identity(gpu, wrap, key, dtype):
    """Twin handles through a full update, P alone, A alone and back to step 1 (k = 1, 2, 2, 1); the last solve asks for reuseFactor and still factorises."""
    kw = mc.solve_kw(key)
    with make(gpu, key, dtype) as a, make(gpu, key, dtype) as b:
        before = b.pattern()
        first = run(a, **kw)
        assert same(run(b, **kw), first)
        for what, kP, kA, reuse in (("full", 1, 1, False), ("P alone", 2, None, False), ("A alone", None, 2, False), ("full again", 1, 1, True)):
            mP = None if kP is None else mc.matrices(key, kP)[0]
            mA = None if kA is None else mc.matrices(key, kA)[1]
            a.update_matrices(mP, mA)
            b.update_values(None if kP is None else wrap(vc.values(key, kP)[0]), None if kA is None else wrap(vc.values(key, kA)[1]))
            ra, rb = run(a, reuseFactor=reuse, **kw), run(b, reuseFactor=reuse, **kw)
            print(key, dtype, what, "iterations", [i["iterations"] for i in rb["infos"]][:6], "resPrim", rb["infos"][0]["resPrim"], ra["infos"][0]["resPrim"])
            assert same(rb, ra), what
            if what == "full":
                assert not np.array_equal(rb["X"], first["X"])             # the values did change the problem
        assert all(np.array_equal(p, q) for p, q in zip(b.pattern(), before))


def options_carried(gpu, wrap, key, column_rho=False):
    _, _, Q, L, U = mc.data(key)
    kw = mc.solve_kw(key)
    vS = gpu.equality_rho_scale(L, U, 1e2)
    vS[0] = 10.0
    out = []
    for values_only in (False, True):
        with make(gpu, key) as h:
            h.set_rho_scale(vS)
            h.set_column_rho(True) if column_rho else h.set_adaptive_rho(True)
            h.set_warm_start("state")
            r1 = run(h, **kw)
            if values_only:
                h.update_values(*(wrap(v) for v in vc.values(key, 1)))
            else:
                h.update_matrices(*mc.matrices(key, 1))
            out.append((r1, run(h, r1["X"], **kw)))
    (r1a, r2a), (r1b, r2b) = out
    assert same(r1a, r1b) and same(r2b, r2a)
    assert not np.array_equal(r2a["X"], r1a["X"])


def equilibrated(gpu, wrap):
    key = mc.SCRAMBLED_SPARSE
    kw = mc.solve_kw(key)
    with make(gpu, key) as a, make(gpu, key) as b:
        for h in (a, b):
            h.set_equilibration(mc.PASSES)
            run(h, **kw)
        D, E = b.equilibration()
        assert (D != 1).any() and (E != 1).any()
        a.update_matrices(*mc.matrices(key, 1))
        b.update_values(*(wrap(v) for v in vc.values(key, 1)))
        D2, E2 = b.equilibration()
        assert np.array_equal(D, D2) and np.array_equal(E, E2)
        assert same(run(b, **kw), run(a, **kw))
        b.set_equilibration(mc.PASSES)                                     # computed from the host copies: they have to hold the new values
        Dn, En = b.equilibration()
        again = run(b, **kw)
    with getattr(gpu, vc.CLASSES["sparse"])(*mc.matrices(key, 1), *mc.data(key)[2:]) as f:
        f.set_equilibration(mc.PASSES)
        Df, Ef = f.equilibration()
        want = run(f, **kw)
    assert not (np.array_equal(Df, D) and np.array_equal(Ef, E))          # the new matrices do ask for another scaling
    assert np.array_equal(Dn, Df) and np.array_equal(En, Ef)
    assert same(again, want)


class Untouched:
    """A handle after one solve, and the proof that a refused call left it alone: the re-solve with reuseFactor equals the first solve (which equals that of
    a twin nobody touched), the exponents and the certificate are what they were."""

    def __init__(self, gpu, h, kw, twin):
        self.h, self.kw = h, kw
        self.before = run(h, **kw)
        assert same(self.before, twin)
        self.eq, self.cert = h.equilibration(), h.certificate()

    def check(self, what):
        assert same(run(self.h, reuseFactor=True, **self.kw), self.before), what
        assert all(np.array_equal(p, q) for p, q in zip(self.h.equilibration(), self.eq)), what
        assert all(np.array_equal(p, q) for p, q in zip(self.h.certificate(), self.cert)), what


def same_refusal(h, M_P, M_A, vP, vA, wrap, rename=False):
    """update_matrices and update_values refuse the same values with the same status and text (rename: but for the function name in the range message)."""
    want = refusal(lambda: h.update_matrices(M_P, M_A))
    got = refusal(lambda: h.update_values(None if vP is None else wrap(vP), None if vA is None else wrap(vA)))
    if rename:
        want = (want[0], want[1].replace("qps_update_shared_matrices_csc", "qps_update_shared_values"))
    print(got)
    assert got == want, (got, want)
    return got


def twin_solve(gpu, key, dtype="f64", P=None, kw=None):
    with make(gpu, key, dtype, P) as t:
        return run(t, **(kw or mc.solve_kw(key)))


def refused_values(gpu, wrap):
    """NaN / Inf and asymmetric values on the handles of mc.RANDOM and mc.CG_SMALL."""
    twins = {key: twin_solve(gpu, key) for key in (mc.RANDOM, mc.CG_SMALL)}
    handles = {key: make(gpu, key) for key in twins}
    try:
        guard = {key: Untouched(gpu, h, mc.solve_kw(key), twins[key]) for key, h in handles.items()}
        for name, key, vP, vA, _ in vc.not_finite_cases():
            P0, A0 = mc.matrices(key, 0)
            status, msg = same_refusal(handles[key], vc.with_values(P0, vP), None if vA is None else vc.with_values(A0, vA), vP, vA, wrap)
            assert status == NOT_FINITE and msg == ("P contains NaN/Inf" if vA is None else "A contains NaN/Inf"), (name, status, msg)
            guard[key].check(name)
        c = mc.canonical(mc.matrices(mc.RANDOM, 0)[0])
        for name, vP, _ in vc.asymmetric_cases():
            status, msg = same_refusal(handles[mc.RANDOM], vc.with_values(c, vP), None, vP, None, wrap)
            assert status == BAD_ARGUMENT and f"(asymmetric entry in column {vc.reported_column(c, vP)})" in msg, (name, status, msg)
            guard[mc.RANDOM].check(name)
    finally:
        for h in handles.values():
            h.close()


def one_sided(gpu, wrap, kind):
    P1, k0, i, j = vc.one_sided()
    key = mc.RANDOM
    cls = getattr(gpu, vc.CLASSES[kind])
    _, A0, Q, L, U = mc.data(key)
    c = mc.canonical(P1)
    with cls(P1, A0, Q, L, U) as t:
        twin = run(t, **vc.FIXED)
    with cls(P1, A0, Q, L, U) as h, cls(P1, A0, Q, L, U) as a:
        guard = Untouched(gpu, h, vc.FIXED, twin)
        assert h.pattern()[1][k0] == i and np.array_equal(h.pattern()[1], c.indices)          # the explicit zero is part of the pattern
        v = c.data.copy()
        v[k0] = 0.25
        status, msg = same_refusal(h, vc.with_values(c, v), None, v, None, wrap)
        assert status == BAD_ARGUMENT and f"(asymmetric entry in column {i})" in msg, (status, msg)          # column j holds it, column i < j is named
        guard.check("one-sided non-zero")
        run(a, **vc.FIXED)
        for zero in (0.0, -0.0):
            v[k0] = zero
            h.update_values(wrap(v))
            a.update_matrices(vc.with_values(c, v))
            assert same(run(h, **vc.FIXED), run(a, **vc.FIXED)), zero


def range_refused(gpu, wrap):
    P, A1, A2, Q, L, U = mc.range_case()
    kw = dict(numIterations=50, ϵAbs=0.0, ϵRel=0.0, ρ=mc.RHO)
    cls = gpu.QuadraticProgramSparseSharedBatch
    with cls(sp.csc_matrix(P), sp.csc_matrix(A1), Q, L, U, dtype="f32") as t:
        t.set_equilibration(mc.PASSES)
        twin = run(t, **kw)
    with cls(sp.csc_matrix(P), sp.csc_matrix(A1), Q, L, U, dtype="f32") as h:
        h.set_equilibration(mc.PASSES)
        guard = Untouched(gpu, h, kw, twin)
        vA = mc.canonical(sp.csc_matrix(A2)).data.copy()
        status, msg = same_refusal(h, None, sp.csc_matrix(A2), None, vA, wrap, rename=True)
        assert status == UNSUPPORTED and msg.startswith("qps_update_shared_values: a scaled matrix entry would leave the normal range") and \
            "the handle is unchanged" in msg, (status, msg)
        guard.check("range")
    with cls(sp.csc_matrix(P), sp.csc_matrix(A1), Q, L, U, dtype="f64") as h:          # the same values on an fp64 handle are in range
        h.set_equilibration(mc.PASSES)
        h.update_values(vA=wrap(vA))


def certificate_kept_and_cleared(gpu, wrap):
    """A handle that holds a certificate: a refused update leaves it, a committed one clears it until the next solve."""
    import infeasibility_cases as ic
    name = "sparse-primal-r1"
    P, A, Q, L, U = ic.case_data(name)
    kw = dict(numIterations=5000, ϵAbs=1e-6, ϵRel=1e-6, ρ=1.0)
    with gpu.QuadraticProgramSparseSharedBatch(P, A, Q, L, U) as h:
        h.set_infeasibility(1e-4, 1e-4)
        _, flags, _ = h.solve(**kw)
        assert [int(f) for f in flags] == ic.CASES[name]["flags"] and 4 in [int(f) for f in flags]
        DY, DX = h.certificate()
        assert DY.any()
        vP = mc.canonical(P).data.copy()
        bad = vP.copy()
        bad[len(bad) // 2] = np.nan
        assert refusal(lambda: h.update_values(wrap(bad)))[0] == NOT_FINITE
        assert np.array_equal(h.certificate()[0], DY) and np.array_equal(h.certificate()[1], DX)
        h.update_values(wrap(vP))
        assert not h.certificate()[0].any() and not h.certificate()[1].any()
        _, flags, _ = h.solve(**kw)
        assert np.array_equal(h.certificate()[0], DY)                     # the same values: the same certificate again


CHECKS = {}
for _key in vc.KEYS:
    CHECKS[f"identity-{'-'.join(map(str, _key))}-f64"] = (identity, (_key, "f64"))
for _key in vc.F32_KEYS:
    CHECKS[f"identity-{'-'.join(map(str, _key))}-f32"] = (identity, (_key, "f32"))
CHECKS["options-sparse"] = (options_carried, (mc.RANDOM,))
CHECKS["options-cg-family-rule"] = (options_carried, (mc.CG_BANDED,))
CHECKS["options-cg-column-rho"] = (options_carried, (mc.CG_BANDED, True))
CHECKS["equilibrated"] = (equilibrated, ())
CHECKS["refused-values"] = (refused_values, ())
CHECKS["one-sided-sparse"] = (one_sided, ("sparse",))
CHECKS["one-sided-cg"] = (one_sided, ("cg",))
CHECKS["range"] = (range_refused, ())
CHECKS["certificate"] = (certificate_kept_and_cleared, ())
