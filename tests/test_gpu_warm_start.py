"""Opt-in warm start of z and y of the shared-matrix batches on the device (qps_set_shared_warm_start, qps_set_shared_dual): mode 1 continues every column from the
z and y the handle holds, mode 2 takes y from the handle and forms z = A x on the device, mode 0 -- the default -- is the cold start.  The reference is the numpy
restatement of tests/warm_start_cases.py with the state passed in: its reduced Cholesky form for the dense handle, its dense KKT form for the sparse one.
Base rho = 0.1 throughout.

Bounds are those of tests/test_gpu_rho_scale.py for the same families: dense fp64 and sparse random 1e-9 relative on x and z, 1e-8 on y, residuals 1e-8; the
lasso path 1e-6 / 1e-5; fp32 1e-3 on x; flags and iteration counts equal per column."""
import ctypes as C

import numpy as np
import pytest

import equilibration_cases as ec
import warm_start_cases as wc
from test_gpu_parity import rel

pytestmark = pytest.mark.gpu

BAD_ARGUMENT, UNSUPPORTED = 1, 8
RHO = 0.1
FIXED = dict(ϵAbs=0.0, ϵRel=0.0, ρ=RHO)
INFO_KEYS = ("convFlag", "iterations", "numRefactor", "cgIterations", "rhoFinal", "rhoProposed", "resPrim", "resDual", "polishFlag", "polishIterations", "trsvBlock",
             "sweepVariant", "sweepGaveUp", "cgExplicit")          # every field of qps_info but the four wall times

CACHED, STAGED = ("shared", 96, 160, 4), ("shared", 2112, 2304, 37)          # 16-wave cached form; staged form on three panels: a pair and a single
STAGED_COLS = (0, 15, 16, 31, 32, 36)
RANDOM, LASSO = ("random", 20), ("lasso", 10, 6)
SCRAMBLED = ("scrambled", 96, 160, 4)


def data(key):
    return ec.family(*key) if key[0] == "scrambled" else wc.family(*key)


def is_sparse(key):
    return key[0] in ("random", "lasso")


@pytest.fixture(scope="module")
def handles(gpu):
    """One handle per (family, type), created at first use and shared by the tests of this module; ``get`` hands it out with every option cleared and the
    family's own q, l, u loaded."""
    made = {}

    def get(key, dtype="f64"):
        P, A, Q, L, U = data(key)
        if (key, dtype) not in made:
            cls = gpu.QuadraticProgramSparseSharedBatch if is_sparse(key) else gpu.QuadraticProgramSharedBatch
            made[(key, dtype)] = [cls(P, A, Q, L, U, dtype=dtype), False]
        prob, dirty = made[(key, dtype)]
        prob.set_warm_start(None)
        prob.set_adaptive_rho(False)
        if dirty:                                    # a scale or a scaling was set by the test before (either change costs a factorisation)
            prob.set_rho_scale(None)
            prob.set_equilibration(0)
            made[(key, dtype)][1] = False
        prob.update(Q, L, U)
        return prob

    def mark_dirty(key, dtype="f64"):
        made[(key, dtype)][1] = True

    get.mark_dirty = mark_dirty
    yield get
    for prob, _ in made.values():
        prob.close()


def run(prob, X=None, **kw):
    X, flags, infos = prob.solve(X, **kw)
    Z, Y = prob.dual()
    return dict(X=X, Z=Z, Y=Y, flags=[int(f) for f in flags], infos=infos)


def same(a, b):
    return (all(np.array_equal(a[k], b[k]) for k in ("X", "Z", "Y")) and a["flags"] == b["flags"]
            and all(repr(i[k]) == repr(j[k]) for i, j in zip(a["infos"], b["infos"]) for k in INFO_KEYS))          # repr: NaN residuals compare equal


_REF = {}


def reference(tag, key, passes, kind, form, make):
    """A restatement run, computed once per tag and shared; ``make(R, Q, L, U)`` produces it from the restatement of (family, passes, scale kind, form)."""
    k = (tag, key, passes, kind, form)
    if k not in _REF:
        P, A, Q, L, U = data(key)
        from quadraticprogramsolver_amd import equality_rho_scale
        vS = equality_rho_scale(L, U) if kind == "equality" else None
        _REF[k] = make(wc.WarmRestatement(P, A, passes, vS, form=form), Q, L, U)
    return _REF[k]


def figures(r, ref, b):
    c = ref["columns"][b]
    return (rel(r["X"][b], c["x"]), rel(r["Z"][b], c["z"]), rel(r["Y"][b], c["y"]), abs(r["infos"][b]["resPrim"] - c["resPrim"]) / max(1.0, c["resPrim"]),
            abs(r["infos"][b]["resDual"] - c["resDual"]) / max(1.0, c["resDual"]))


def hold(what, key, dtype, r, ref, cols, tol=1e-9):
    """Flags and iteration counts equal per column, iterates and residuals within the bounds of the module docstring."""
    for b in cols:
        c, fig = ref["columns"][b], figures(r, ref, b)
        print(f"{what} {key} {dtype} column {b}: flag {r['flags'][b]}/{c['convFlag']} iterations {r['infos'][b]['iterations']}/{c['iterations']} "
              f"rel x {fig[0]:.2e} z {fig[1]:.2e} y {fig[2]:.2e} dresPrim {fig[3]:.2e} dresDual {fig[4]:.2e}")
        assert r["flags"][b] == c["convFlag"] and r["infos"][b]["iterations"] == c["iterations"], (what, key, b)
        if dtype == "f32":
            assert fig[0] <= 1e-3, (what, key, b, fig)
        else:
            assert fig[0] <= tol and fig[1] <= tol and fig[2] <= 10 * tol, (what, key, b, fig)
            assert fig[3] <= 10 * tol and fig[4] <= 10 * tol, (what, key, b, fig)


def columns_of(key):
    return STAGED_COLS if key == STAGED else range(data(key)[2].shape[0])


def form_of(key):
    return "kkt" if is_sparse(key) else "reduced"


# ---------------------------------------------------------------------------------------------------------------------
# 1. a fresh handle holds z = y = 0: mode 1 is the cold start
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [CACHED, RANDOM], ids=["dense", "sparse"])
def test_mode_one_on_a_fresh_handle_is_the_cold_start_bit_for_bit(gpu, handles, key):
    P, A, Q, L, U = data(key)
    kw = dict(numIterations=5000, ϵAbs=1e-6, ϵRel=1e-6, ρ=RHO)
    cold = run(handles(key), **kw)
    cls = gpu.QuadraticProgramSparseSharedBatch if is_sparse(key) else gpu.QuadraticProgramSharedBatch
    with cls(P, A, Q, L, U) as fresh:
        Z0, Y0 = fresh.dual()
        assert not Z0.any() and not Y0.any()          # defined from creation on
        fresh.set_warm_start("state")
        first = run(fresh, **kw)
    print("iterations:", [i["iterations"] for i in first["infos"]])
    assert same(first, cold)
    assert len(set(i["iterations"] for i in cold["infos"])) > 1


# ---------------------------------------------------------------------------------------------------------------------
# 2. split solve: K1 iterations, then K2 more from the handle's state, are K1 + K2 iterations
# ---------------------------------------------------------------------------------------------------------------------
SPLIT = [(CACHED, "f64", 50, 50, 1e-9), (CACHED, "f32", 50, 50, None), (STAGED, "f64", 50, 25, 1e-9), (RANDOM, "f64", 50, 50, 1e-9), (LASSO, "f64", 50, 50, 1e-6)]


@pytest.mark.parametrize("key,dtype,K1,K2,tol", SPLIT, ids=[f"{'x'.join(map(str, k))}-{d}" for k, d, _, _, _ in SPLIT])
def test_split_solve_equals_the_single_run_of_the_restatement(handles, key, dtype, K1, K2, tol):
    prob = handles(key, dtype)
    half = run(prob, numIterations=K1, **FIXED)
    prob.set_warm_start("state")
    rest = run(prob, half["X"], numIterations=K2, reuseFactor=True, **FIXED)
    prob.set_warm_start("off")
    whole = run(prob, numIterations=K1 + K2, reuseFactor=True, **FIXED)
    ref = reference(("cold", K1 + K2), key, 0, None, form_of(key), lambda R, Q, L, U: R.solve_from(Q, L, U, numIterations=K1 + K2, epsAbs=0.0, epsRel=0.0))
    ref = dict(ref, columns=[dict(c, iterations=K2) for c in ref["columns"]])          # the counter restarts at 1: the second solve reports its own K2
    hold("split", key, dtype, rest, ref, columns_of(key), tol)
    print(f"split {key} {dtype}: device split against device single run, max abs x {np.abs(rest['X'] - whole['X']).max():.2e} z "
          f"{np.abs(rest['Z'] - whole['Z']).max():.2e} y {np.abs(rest['Y'] - whole['Y']).max():.2e}  (recorded, not asserted)")
    assert not np.array_equal(rest["X"], half["X"])


# ---------------------------------------------------------------------------------------------------------------------
# 3. mode 2: y from the handle, z = A x on the device
# ---------------------------------------------------------------------------------------------------------------------
MODE2 = [(CACHED, "f64"), (CACHED, "f32"), (STAGED, "f64"), (RANDOM, "f64")]


def _y0(L):
    return 0.05 * np.random.default_rng(3).standard_normal(L.shape)


@pytest.mark.parametrize("kind", [None, "equality"], ids=["scalar-rho", "equality-scale"])
@pytest.mark.parametrize("key,dtype", MODE2, ids=[f"{'x'.join(map(str, k))}-{d}" for k, d in MODE2])
def test_mode_two_starts_from_a_x_and_the_stored_y(gpu, handles, key, dtype, kind):
    P, A, Q, L, U = data(key)
    X0, Y0, K = ec.warm_start(Q), _y0(L), 50
    prob = handles(key, dtype)
    if kind:
        prob.set_rho_scale(gpu.equality_rho_scale(L, U))          # the row-vector form of the start
        handles.mark_dirty(key, dtype)
    prob.set_warm_start("ax")
    prob.set_dual(mY=Y0)
    r = run(prob, X0, numIterations=K, **FIXED)
    ref = reference("ax", key, 0, kind, form_of(key),
                    lambda R, Q, L, U: R.solve_from(Q, L, U, X0, X0 @ wc.dense(A).T, Y0, numIterations=K, epsAbs=0.0, epsRel=0.0))
    hold(f"mode 2 {kind}", key, dtype, r, ref, columns_of(key))
    if key != STAGED:                                     # (one restatement run less at the large shape)
        cold = reference(("cold", K), key, 0, kind, form_of(key), lambda R, Q, L, U: R.solve_from(Q, L, U, numIterations=K, epsAbs=0.0, epsRel=0.0))
        assert rel(ref["X"][0], cold["X"][0]) > 1e-6      # the start matters at K = 50: a cold start would not pass


# ---------------------------------------------------------------------------------------------------------------------
# 4. qps_set_shared_dual is the counterpart of qps_get_dual
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("passes", [0, 10], ids=["unscaled", "equilibrated"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_set_dual_of_dual_changes_no_bit(handles, dtype, passes):
    prob = handles(SCRAMBLED, dtype)
    if passes:
        prob.set_equilibration(passes)
        handles.mark_dirty(SCRAMBLED, dtype)

    def state():          # the same (x, z, y) on the handle every time: the loop is deterministic
        prob.set_warm_start("off")
        half = run(prob, numIterations=50, **FIXED)
        prob.set_warm_start("state")
        return half

    half = state()
    plain = run(prob, half["X"], numIterations=50, reuseFactor=True, **FIXED)
    half2 = state()
    assert same(half2, half)
    prob.set_dual(*prob.dual())
    Z, Y = prob.dual()
    assert np.array_equal(Z, half["Z"]) and np.array_equal(Y, half["Y"])
    assert same(run(prob, half["X"], numIterations=50, reuseFactor=True, **FIXED), plain)
    state()
    prob.set_dual(mZ=None, mY=half["Y"])                        # None keeps z: a zeroed or stale z would change the run
    assert np.array_equal(prob.dual()[0], half["Z"])
    assert same(run(prob, half["X"], numIterations=50, reuseFactor=True, **FIXED), plain)
    state()
    prob.set_dual(mZ=half["Z"])                                  # and y
    assert np.array_equal(prob.dual()[1], half["Y"])
    state()
    prob.set_dual(mY=np.zeros_like(half["Y"]))
    assert not same(run(prob, half["X"], numIterations=50, reuseFactor=True, **FIXED), plain)          # what set_dual writes is what the solve reads


# ---------------------------------------------------------------------------------------------------------------------
# 5. re-solve sequences to eps = 1e-6: update + mode 1 + reuseFactor
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(wc.CASES))
def test_resolve_sequence_follows_the_case_table(handles, name):
    c = wc.CASES[name]
    key, seq = c["family"], wc.sequence_data(name)
    runs = wc.sequence_run(name, c["form"])
    prob = handles(key)
    kw = dict(numIterations=5000, ϵAbs=1e-6, ϵRel=1e-6, ρ=RHO)
    r = run(prob, **kw)
    prob.set_warm_start("state")
    for k in range(len(seq)):
        if k:
            prob.update(*seq[k])
            r = run(prob, r["X"], reuseFactor=True, **kw)
        print(f"{name} step {k}: iterations {[i['iterations'] for i in r['infos']]} tSetup {r['infos'][0]['tSetup'] * 1e3:.3f} ms tLoop {r['infos'][0]['tLoop'] * 1e3:.2f} ms")
        assert [i["iterations"] for i in r["infos"]] == c["iterations"][k] and r["flags"] == c["flags"][k], (name, k)
        hold(f"{name} step {k}", key, "f64", r, runs[k], range(len(r["flags"])))


# ---------------------------------------------------------------------------------------------------------------------
# 6. composition with the other options of the handle
# ---------------------------------------------------------------------------------------------------------------------
def test_equilibration_switched_on_between_two_solves_carries_the_state_over(handles):
    """The second solve runs in other variables (x~ = D^-1 x, z~ = E z, y~ = E^-1 y) and continues from the same caller-unit state: the restatement is started
    from what the handle returned for the first solve."""
    P, A, Q, L, U = data(SCRAMBLED)
    prob = handles(SCRAMBLED)
    half = run(prob, numIterations=50, **FIXED)
    prob.set_equilibration(10)
    handles.mark_dirty(SCRAMBLED)
    Z, Y = prob.dual()
    assert np.array_equal(Z, half["Z"]) and np.array_equal(Y, half["Y"])          # exact powers of two
    prob.set_warm_start("state")
    rest = run(prob, half["X"], numIterations=50, **FIXED)
    ref = wc.WarmRestatement(P, A, 10, form="reduced").solve_from(Q, L, U, half["X"], half["Z"], half["Y"], numIterations=50, epsAbs=0.0, epsRel=0.0)
    hold("equilibration on between solves", SCRAMBLED, "f64", rest, ref, range(4))
    cold = wc.WarmRestatement(P, A, 10, form="reduced").solve_from(Q, L, U, half["X"], numIterations=50, epsAbs=0.0, epsRel=0.0)
    assert rel(ref["Z"][0], cold["Z"][0]) > 1e-6


def test_family_rho_rule_and_a_warm_resolve_at_its_final_rho(handles):
    """set_adaptive_rho(), a cold solve, then the perturbed data re-solved warm at rho = rhoFinal of the longest-running column with reuseFactor: nothing is
    factorised at setup and the run is the restatement's from the handle's state at that rho, under the same rule."""
    P, A, Q, L, U = data(CACHED)
    prob = handles(CACHED)
    prob.set_adaptive_rho()
    first = run(prob, numIterations=5000, ϵAbs=1e-6, ϵRel=1e-6, ρ=RHO, fctrΡ=5)
    longest = max(range(4), key=lambda b: first["infos"][b]["iterations"])
    rho = first["infos"][longest]["rhoFinal"]
    assert first["infos"][longest]["numRefactor"] >= 1 and rho != RHO
    Q2, L2, U2 = wc.step(Q, L, U, 1)
    prob.update(Q2, L2, U2)
    prob.set_warm_start("state")
    prob.set_profiling(1)
    K = 100
    r = run(prob, first["X"], numIterations=K, ϵAbs=0.0, ϵRel=0.0, ρ=rho, fctrΡ=5, reuseFactor=True)
    setup = [k for k in prob.kernel_times() if "factorisation at setup" in k["name"]]
    prob.set_profiling(0)
    assert sum(k["launches"] for k in setup) == 0
    ref = wc.WarmRestatement(P, A, form="reduced").solve_from(Q2, L2, U2, first["X"], first["Z"], first["Y"], rho=rho, numIterations=K, epsAbs=0.0, epsRel=0.0,
                                                              adaptive=True, fctrRho=5.0)
    print(f"rho {rho!r}; switches of the warm re-solve {ref['switches']}; quotients {[f'{q:.3f}' for _, q in ref['quotients']]}")
    hold("family rho, warm re-solve", CACHED, "f64", r, ref, range(4))
    for b in range(4):
        assert r["infos"][b]["numRefactor"] == ref["columns"][b]["numRefactor"]
        assert abs(r["infos"][b]["rhoFinal"] - ref["columns"][b]["rhoFinal"]) <= 1e-10 * ref["columns"][b]["rhoFinal"]


# ---------------------------------------------------------------------------------------------------------------------
# 7. refusals
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [CACHED, RANDOM], ids=["dense", "sparse"])
def test_bad_arguments_are_refused_and_the_handle_keeps_its_state(gpu, handles, key):
    from quadraticprogramsolver_amd import _lib
    prob = handles(key)

    def state():
        prob.set_warm_start("off")
        half = run(prob, numIterations=50, **FIXED)
        prob.set_warm_start("state")
        return half

    half = state()
    plain = run(prob, half["X"], numIterations=50, reuseFactor=True, **FIXED)
    for mode in (3, -1):
        assert _lib.lib().qps_set_shared_warm_start(prob._h, mode) == BAD_ARGUMENT
        with pytest.raises(gpu.QpsError) as e:
            prob.set_warm_start(mode)
        assert e.value.status == BAD_ARGUMENT and "mode" in e.value.message
    for which, bad in (("mZ", np.nan), ("mZ", np.inf), ("mY", np.nan), ("mY", -np.inf)):
        state()
        V = half["Z" if which == "mZ" else "Y"].copy()
        V[-1, -1] = bad
        with pytest.raises(gpu.QpsError) as e:
            prob.set_dual(**{which: V})
        assert e.value.status == BAD_ARGUMENT, (which, bad)
        assert same(run(prob, half["X"], numIterations=50, reuseFactor=True, **FIXED), plain), (which, bad)          # still mode 1, still the stored state
    with pytest.raises(ValueError):
        prob.set_dual(mZ=half["Z"][:, :-1])
    prob.set_warm_start("off")                                   # mode 0 after mode 1: the cold start again
    assert same(run(prob, numIterations=50, reuseFactor=True, **FIXED), half)


def test_other_handles_are_unsupported(gpu):
    from quadraticprogramsolver_amd import _lib
    L_ = _lib.lib()
    P, A, Q, L, U = data(CACHED)
    z = np.zeros(2 * A.shape[0])
    dp = z.ctypes.data_as(C.POINTER(C.c_double))
    with gpu.QuadraticProgram(P, Q[0], A, L[0], U[0]) as one, gpu.QuadraticProgramBatch([(P, Q[b], A, L[b], U[b]) for b in range(2)]) as batch, \
            gpu.ProxQP(P, Q[0], A[:8], np.zeros(8), A[8:], U[0][8:]) as prox:
        for h in (one._h, batch._h, prox._h):
            for mode in (0, 1, 2):
                assert L_.qps_set_shared_warm_start(h, mode) == UNSUPPORTED
                assert b"shared-matrix batch" in L_.qps_last_error(h)
            assert L_.qps_set_shared_dual(h, dp, dp) == UNSUPPORTED
            assert b"shared-matrix batch" in L_.qps_last_error(h)
            assert L_.qps_set_shared_dual(h, None, None) == UNSUPPORTED
            assert L_.qps_set_shared_warm_start(h, 3) == BAD_ARGUMENT and L_.qps_set_shared_warm_start(h, -1) == BAD_ARGUMENT          # the argument is judged first
