"""Shared-matrix batch on the device (qps_create_dense_shared_batch): every column of a family that shares mP and mA behaves as a
stand-alone solve of the C oracle on (P, q_b, A, l_b, u_b) with a fixed rho."""
import numpy as np
import pytest

from shared_batch_cases import shared_family
from test_gpu_parity import ABS_DEV_THR, rel

pytestmark = pytest.mark.gpu

UNSUPPORTED = 8


def _oracle(c_oracle, P, A, Q, L, U, b, **kw):
    return c_oracle.solve(P, Q[b], A, L[b], U[b], rho=0.1, **kw)


@pytest.mark.parametrize("n,m,count", [(96, 160, 6), (1100, 2300, 20)])   # the second: two panels, a ragged last one
def test_fixed_k_iterates_match_the_oracle_per_column(gpu, c_oracle, n, m, count):
    """eps 0, K = 100, rho = 0.1, fp64: the bounds of test_iterates_match_oracle_all_classes, for every column."""
    P, A, Q, L, U = shared_family(n, m, count)
    with gpu.QuadraticProgramSharedBatch(P, A, Q, L, U) as prob:
        X, flags, infos = prob.solve(numIterations=100, ϵAbs=0.0, ϵRel=0.0, ρ=0.1)
        Z, Y = prob.dual()
    assert X.shape == (count, n) and Z.shape == (count, m) and Y.shape == (count, m)
    for b in range(count):
        xo, io = _oracle(c_oracle, P, A, Q, L, U, b, numIterations=100, epsAbs=0.0, epsRel=0.0)
        fig = (rel(X[b], xo), rel(Z[b], io["z"]), rel(Y[b], io["y"]), abs(infos[b]["resPrim"] - io["resPrim"]), abs(infos[b]["resDual"] - io["resDual"]))
        print(f"n={n} m={m} column {b}: rel x {fig[0]:.2e} z {fig[1]:.2e} y {fig[2]:.2e} |dresPrim| {fig[3]:.2e} |dresDual| {fig[4]:.2e}")
        assert flags[b] == gpu.ConvergenceFlag.convNumItr and infos[b]["iterations"] == 100
        assert fig[0] <= 1e-9 and fig[1] <= 1e-9 and fig[2] <= 1e-8
        assert fig[3] <= 1e-9 * max(1.0, io["resPrim"])
        assert fig[4] <= 1e-9 * max(1.0, io["resDual"])


def test_every_column_stops_at_its_own_iteration(gpu, c_oracle):
    """To eps = 1e-6 with rho = 0.1: flag and iteration count of every column equal the oracle's, x within ABS_DEV_THR, and the columns do not
    all stop at the same check (a stopped column is frozen while the others go on)."""
    n, m, count = 96, 160, 6
    P, A, Q, L, U = shared_family(n, m, count)
    with gpu.QuadraticProgramSharedBatch(P, A, Q, L, U) as prob:
        X, flags, infos = prob.solve(ϵAbs=1e-6, ϵRel=1e-6, ρ=0.1)
    its = []
    for b in range(count):
        xo, io = _oracle(c_oracle, P, A, Q, L, U, b, numIterations=5000, epsAbs=1e-6, epsRel=1e-6)
        dev = np.abs(X[b] - xo).max()
        print(f"column {b}: flag {int(flags[b])}/{io['convFlag']} iterations {infos[b]['iterations']}/{io['iterations']} max|x - x_oracle| {dev:.2e}")
        assert int(flags[b]) == io["convFlag"] and infos[b]["iterations"] == io["iterations"]
        assert dev <= ABS_DEV_THR
        its.append(infos[b]["iterations"])
    assert len(set(its)) > 1, its


def test_columns_are_independent_and_runs_repeat_bit_for_bit(gpu):
    """Each MFMA output element is its own dot product: column b of a count-20 solve equals, bit for bit, the same data solved in a count-1
    shared handle; two runs of one solve are bit-identical."""
    n, m, count = 200, 330, 20
    P, A, Q, L, U = shared_family(n, m, count)
    kw = dict(numIterations=150, ϵAbs=1e-4, ϵRel=1e-4, ρ=0.1)      # some columns stop early, others run all 150
    with gpu.QuadraticProgramSharedBatch(P, A, Q, L, U) as prob:
        X, flags, infos = prob.solve(**kw)
        Z, Y = prob.dual()
        X2, flags2, infos2 = prob.solve(**kw)
        Z2, Y2 = prob.dual()
    assert np.array_equal(X, X2) and np.array_equal(Z, Z2) and np.array_equal(Y, Y2)
    assert [i["iterations"] for i in infos] == [i["iterations"] for i in infos2]
    for b in (0, 1, 7, 15, 16, 19):                                 # both panels, first and last column of each
        with gpu.QuadraticProgramSharedBatch(P, A, Q[b:b + 1], L[b:b + 1], U[b:b + 1]) as one:
            x1, f1, i1 = one.solve(**kw)
            z1, y1 = one.dual()
        assert f1[0] == flags[b] and i1[0]["iterations"] == infos[b]["iterations"]
        assert np.array_equal(x1[0], X[b]) and np.array_equal(z1[0], Z[b]) and np.array_equal(y1[0], Y[b]), b


def test_vector_update_keeps_the_factorisation(gpu):
    """update() followed by solve(reuseFactor=True) equals a freshly created handle on the new vectors bit for bit, and its tSetup shows no
    factorisation.  At n = 2048, m = 4096 the first solve's setup forms A'A (2 m n^2 = 34 GFLOP), factorises (n^3 / 3) and inverts the factor
    (n^3 / 3): 40 GFLOP of fp64, at least half a millisecond even at the chip's matrix peak.  The reused setup uploads count * n warm starts and
    clears the state: a dozen launch-bound calls.  Half of the first solve's time separates the two with a wide margin on either side."""
    n, m, count = 2048, 4096, 5
    P, A, Q, L, U = shared_family(n, m, count)
    _, _, Q2, L2, U2 = shared_family(n, m, count, stream=4)
    kw = dict(numIterations=50, ϵAbs=0.0, ϵRel=0.0, ρ=0.1)
    with gpu.QuadraticProgramSharedBatch(P, A, Q, L, U) as prob:
        _, _, first = prob.solve(**kw)
        prob.update(Q2, L2, U2)
        X, flags, infos = prob.solve(reuseFactor=True, **kw)
        Z, Y = prob.dual()
        prob.update(mQ=Q)                                            # a partial update: only q changes
        Xq, _, _ = prob.solve(reuseFactor=True, **kw)
    with gpu.QuadraticProgramSharedBatch(P, A, Q2, L2, U2) as fresh:
        Xf, _, _ = fresh.solve(**kw)
        Zf, Yf = fresh.dual()
    with gpu.QuadraticProgramSharedBatch(P, A, Q, L2, U2) as fresh_q:
        Xfq, _, _ = fresh_q.solve(**kw)
    assert np.array_equal(X, Xf) and np.array_equal(Z, Zf) and np.array_equal(Y, Yf)
    assert np.array_equal(Xq, Xfq)
    print(f"tSetup first {first[0]['tSetup'] * 1e3:.3f} ms, reused {infos[0]['tSetup'] * 1e3:.3f} ms")
    assert infos[0]["tSetup"] < 0.5 * first[0]["tSetup"]


def test_fp32_shared_batch(gpu, c_oracle):
    """The tolerances of test_fp32_path: 1e-3 relative on the iterates at a fixed K, 1e-3 on the solution to eps = 1e-4."""
    n, m, count = 256, 512, 4
    P, A, Q, L, U = shared_family(n, m, count)
    with gpu.QuadraticProgramSharedBatch(P, A, Q, L, U, dtype="f32") as prob:
        X, _, infos = prob.solve(numIterations=50, ϵAbs=0.0, ϵRel=0.0, ρ=0.1)
        Xe, flags, _ = prob.solve(numIterations=2000, ϵAbs=1e-4, ϵRel=1e-4, ρ=0.1, numItrConv=50)
    for b in range(count):
        xo, _ = _oracle(c_oracle, P, A, Q, L, U, b, numIterations=50, epsAbs=0.0, epsRel=0.0)
        xe, _ = _oracle(c_oracle, P, A, Q, L, U, b, numIterations=2000, epsAbs=1e-4, epsRel=1e-4, numItrConv=50)
        print(f"fp32 column {b}: rel x at K = 50 {rel(X[b], xo):.2e}, max|x - x_oracle| to eps {np.abs(Xe[b] - xe).max():.2e}")
        assert infos[b]["iterations"] == 50 and rel(X[b], xo) <= 1e-3
        assert int(flags[b]) in (2, 3)
        assert np.abs(Xe[b] - xe).max() <= 1e-3 * max(1.0, np.abs(xe).max())


def test_unsupported_requests_are_refused_and_the_handle_stays_usable(gpu, c_oracle):
    n, m, count = 96, 160, 3
    P, A, Q, L, U = shared_family(n, m, count)
    with gpu.QuadraticProgramSharedBatch(P, A, Q, L, U) as prob:
        for kw, word in ((dict(adptΡ=True), "adptRho"), (dict(polish=True), "polish"), (dict(trsvBlock=64), "trsvBlock")):
            with pytest.raises(gpu.QpsError) as e:
                prob.solve(ρ=0.1, **kw)
            assert e.value.status == UNSUPPORTED and word in e.value.message, (kw, e.value.message)
        X, flags, infos = prob.solve(numIterations=100, ϵAbs=0.0, ϵRel=0.0, ρ=0.1, trsvBlock=128)   # trsvBlock >= n is accepted
        for b in range(count):
            xo, _ = _oracle(c_oracle, P, A, Q, L, U, b, numIterations=100, epsAbs=0.0, epsRel=0.0)
            assert rel(X[b], xo) <= 1e-9


# ---------------------------------------------------------------------------------------------------------------------
# Matrices above the 32 MiB cut of shared_panel_small run the STAGED kernel form (whole-row loads turned into operand layout through the
# wave's LDS tile, 8 waves, two panels per workgroup).  The shapes below put A, A', P and S above the cut (n > 2048 in fp64) and take three
# panels, so the two-panel instantiations, their ragged last group and the staged triangular sweeps all run -- against the C oracle and
# against a count-1 handle (one panel per workgroup).
# ---------------------------------------------------------------------------------------------------------------------
def test_staged_kernels_match_the_oracle_and_a_single_column_handle(gpu, c_oracle):
    n, m, count = 2112, 2304, 37            # A 38.9 MB, S and P 35.7 MB in fp64; 3 panels: a pair and a ragged single
    P, A, Q, L, U = shared_family(n, m, count)
    fixed = dict(numIterations=50, ϵAbs=0.0, ϵRel=0.0, ρ=0.1)
    early = dict(numIterations=200, ϵAbs=1e-3, ϵRel=1e-3, ρ=0.1)
    with gpu.QuadraticProgramSharedBatch(P, A, Q, L, U) as prob:
        X, flags, infos = prob.solve(**fixed)
        Z, Y = prob.dual()
        Xe, flags_e, infos_e = prob.solve(reuseFactor=True, **early)
    for b in (0, 5, 15, 16, 20, 31, 32, 36):                       # every panel, first and last column of each
        xo, io = _oracle(c_oracle, P, A, Q, L, U, b, numIterations=50, epsAbs=0.0, epsRel=0.0)
        fig = (rel(X[b], xo), rel(Z[b], io["z"]), rel(Y[b], io["y"]), abs(infos[b]["resPrim"] - io["resPrim"]), abs(infos[b]["resDual"] - io["resDual"]))
        print(f"staged n={n} m={m} column {b}: rel x {fig[0]:.2e} z {fig[1]:.2e} y {fig[2]:.2e} |dresPrim| {fig[3]:.2e} |dresDual| {fig[4]:.2e}")
        assert flags[b] == gpu.ConvergenceFlag.convNumItr and infos[b]["iterations"] == 50
        assert fig[0] <= 1e-9 and fig[1] <= 1e-9 and fig[2] <= 1e-8
        assert fig[3] <= 1e-9 * max(1.0, io["resPrim"])
        assert fig[4] <= 1e-9 * max(1.0, io["resDual"])
    its = []
    for b in (1, 16, 33, 36):                                       # column 1 has l = -Inf; to a tolerance, every column on its own
        xo, io = _oracle(c_oracle, P, A, Q, L, U, b, numIterations=200, epsAbs=1e-3, epsRel=1e-3)
        dev = np.abs(Xe[b] - xo).max()
        print(f"staged column {b}: flag {int(flags_e[b])}/{io['convFlag']} iterations {infos_e[b]['iterations']}/{io['iterations']} max|x - x_oracle| {dev:.2e}")
        assert int(flags_e[b]) == io["convFlag"] and infos_e[b]["iterations"] == io["iterations"]
        assert dev <= ABS_DEV_THR
        its.append(infos_e[b]["iterations"])
    print("stopping iterations of the whole batch:", sorted(set(i["iterations"] for i in infos_e)))
    for b in (0, 17, 36):                                           # two panels per workgroup against one: bit for bit
        with gpu.QuadraticProgramSharedBatch(P, A, Q[b:b + 1], L[b:b + 1], U[b:b + 1]) as one:
            x1, f1, i1 = one.solve(**fixed)
            z1, y1 = one.dual()
            xe1, fe1, ie1 = one.solve(reuseFactor=True, **early)
        assert np.array_equal(x1[0], X[b]) and np.array_equal(z1[0], Z[b]) and np.array_equal(y1[0], Y[b]), b
        assert fe1[0] == flags_e[b] and ie1[0]["iterations"] == infos_e[b]["iterations"] and np.array_equal(xe1[0], Xe[b]), b


def test_staged_kernels_fp32(gpu, c_oracle):
    """fp32 above the cut (A 37 MB, S and P 36 MB), three panels: the fixed-K tolerance of test_fp32_path against the fp64 oracle."""
    n, m, count = 3008, 3072, 33
    P, A, Q, L, U = shared_family(n, m, count)
    kw = dict(numIterations=50, ϵAbs=0.0, ϵRel=0.0, ρ=0.1)
    with gpu.QuadraticProgramSharedBatch(P, A, Q, L, U, dtype="f32") as prob:
        X, _, infos = prob.solve(**kw)
    for b in (0, 16, 32):
        xo, _ = _oracle(c_oracle, P, A, Q, L, U, b, numIterations=50, epsAbs=0.0, epsRel=0.0)
        print(f"staged fp32 column {b}: rel x at K = 50 {rel(X[b], xo):.2e}")
        assert infos[b]["iterations"] == 50 and rel(X[b], xo) <= 1e-3
    with gpu.QuadraticProgramSharedBatch(P, A, Q[32:33], L[32:33], U[32:33], dtype="f32") as one:
        x1, _, _ = one.solve(**kw)
    assert np.array_equal(x1[0], X[32])
