"""The setup chain of the dense solvers (k_setup.hip through DenseChol: A'A, M = P + σI + ρA'A, the Cholesky chain, the explicit inverse by recursive doubling,
the premultiplied form) in every band of the padded order, both types, on systems whose exact solution x* is known: tests/setup_band_cases.py holds the
systems, the case table with the branch every case reaches, the bound (8 x the error of the numpy restatement and of LAPACK in the type; nothing from GPU
output) and the figures measured on an MI355X; tests/test_setup_bands_cpu.py checks on the CPU that the systems are exact, that the bound follows from the
restatement, that a wrong tile of L or A'A moves x by 1000 x the bound, and that the table reaches both sides of every threshold.  Stand-alone handles go
through the plugin pair (linsys_init / linsys_solve with x = z = y = 0: x~ = x*, z~ = A x*), the batch through one iteration at α = 1 from a zero start.
The breakdown tests feed finite matrices with one negative pivot and expect QPS_ERR_FACTORIZATION naming the column.  Every figure is printed before its
assertion (run with -s)."""
import re
import time

import numpy as np
import pytest

import setup_band_cases as S

pytestmark = pytest.mark.gpu


def _plugin_solve(h, pr, dtype, rho, changed, tag, t0):
    xx, zz = np.zeros(pr.n), np.zeros(pr.m)
    h.linsys_solve(pr.x_for_rho(rho), np.zeros(pr.m), np.zeros(pr.m), rho, S.SIGMA, changed, xx, zz)
    ex, ez, zb = S.xerr(xx, pr), float(np.abs(zz - pr.A @ pr.xs).max()), pr.zbound(dtype)
    print(f"{tag}: x {ex:.2e}/{S.BOUND[dtype]:.1e} z {ez:.2e}/{zb:.1e} wall {time.perf_counter() - t0:.1f} s")
    assert ex <= S.BOUND[dtype], (tag, ex, S.BOUND[dtype])
    assert ez <= zb, (tag, ez, zb)


@pytest.mark.parametrize("dtype", S.DTYPES)
@pytest.mark.parametrize("case", S.SINGLE, ids=S.single_id)
def test_plugin_pair_returns_the_exact_solution(gpu, case, dtype):
    t0 = time.perf_counter()
    pr, tag = S.problem(case.n, case.m), f"{S.single_id(case)} {dtype}"
    h = gpu.QuadraticProgram(pr.P, pr.q, pr.A, pr.l, pr.u, dtype=dtype)
    try:
        h.linsys_init(S.RHO, S.SIGMA)
        _plugin_solve(h, pr, dtype, S.RHO, False, tag, t0)
        if case.n in S.RHO_SWITCH:                                          # the refactor that reuses the cached A'A, there and back
            _plugin_solve(h, pr, dtype, S.RHO2, True, tag + " rho 2", t0)
            _plugin_solve(h, pr, dtype, S.RHO, True, tag + " rho back", t0)
        for nb in S.TRSV.get(case.n, {}).get(dtype, ()):
            h.linsys_init(S.RHO, S.SIGMA, trsvBlock=nb)
            _plugin_solve(h, pr, dtype, S.RHO, False, f"{tag} trsvBlock {nb}", t0)
    finally:
        h.close()


@pytest.mark.parametrize("dtype", S.DTYPES)
@pytest.mark.parametrize("case", S.BATCH, ids=S.batch_id)
def test_batch_returns_the_exact_solution_of_every_qp(gpu, case, dtype):
    t0 = time.perf_counter()
    prs = S.batch_problems(case)
    h = gpu.QuadraticProgramBatch([(p.P, p.q, p.A, p.l, p.u) for p in prs], dtype=dtype)
    try:
        X, _, infos = h.solve(numIterations=1, ρ=S.RHO, σ=S.SIGMA, α=1.0)    # z = y = 0 and α = 1: the returned x is x~
    finally:
        h.close()
    errs = [S.xerr(X[b], pr) for b, pr in enumerate(prs)]
    print(f"{S.batch_id(case)} {dtype}: x " + " ".join(f"{e:.2e}" for e in errs) + f" /{S.BOUND[dtype]:.1e} wall {time.perf_counter() - t0:.1f} s")
    assert [i["iterations"] for i in infos] == [1] * case.count
    for b, e in enumerate(errs):
        assert e <= S.BOUND[dtype], (S.batch_id(case), dtype, b, e, S.BOUND[dtype])


@pytest.mark.parametrize("dtype", S.DTYPES)
@pytest.mark.parametrize("case", S.BREAKDOWN, ids=S.breakdown_id)
def test_breakdown_is_reported_with_its_column(gpu, case, dtype):
    """Finite input, an ordinary status code: the first non-positive pivot is column c, reported 1-based (PotrfCol); the handle closes afterwards."""
    base, P = S.breakdown_problem(case)
    if case.count == 1:
        pr = base[0]
        h = gpu.QuadraticProgram(P, pr.q, pr.A, pr.l, pr.u, dtype=dtype)
        run = lambda: h.linsys_init(S.RHO, S.SIGMA)
    else:
        h = gpu.QuadraticProgramBatch([(P if b == case.qp else p.P, p.q, p.A, p.l, p.u) for b, p in enumerate(base)], dtype=dtype)
        run = lambda: h.solve(numIterations=1, ρ=S.RHO, σ=S.SIGMA, α=1.0)
    try:
        with pytest.raises(gpu.QpsError) as e:
            run()
        print(f"{S.breakdown_id(case)} {dtype}: status {e.value.status}: {e.value.message}")
        assert e.value.status == 4, e.value                                 # QPS_ERR_FACTORIZATION
        col = re.search(r"non-positive pivot at column (\d+)", e.value.message)
        assert col and int(col.group(1)) == case.c + 1, e.value.message
        assert case.count == 1 or f"QP {case.qp} of the batch" in e.value.message, e.value.message
    finally:
        h.close()
    assert h._h is None
