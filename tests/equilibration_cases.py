"""The opt-in Ruiz equilibration of the shared-matrix batches (qps_set_shared_equilibration) restated in numpy, and the families its tests use.  Plain importable
helper, no device needed: tests/test_equilibration_cpu.py guards it, tests/test_gpu_equilibration.py and tests/tools/gpu_equilibration_timing.py compare the
device with it.

The scaling is D = diag(2^kd) on the variables and E = diag(2^ke) on the constraints, exponents by ``ruiz_pow2`` (integer arithmetic on exponents only, so numpy
and the device agree exactly).  The loop is the batch loop of tests/family_rho_cases.py on  P~ = D P D, A~ = E A D, q~ = D q, l~ = E l, u~ = E u  in the reduced
Cholesky form (dense handle) or the dense KKT form (sparse handle); CheckConvergence and the family-wide rho rule see the unscaled D x~, E^-1 z~, E y~ (OSQP 5.1).
In the original variables that loop is ADMM with sigma_j = sigma / D_j^2 and rho_i = rho E_i^2, which is why its iterates differ from an unscaled solve."""
import math

import numpy as np
import scipy.sparse as sp

from family_rho_cases import FamilyRestatement, family_proposal
from oracle.qps_oracle_np import CheckConvergence, ConvergenceFlag, _jclamp, _jmax, _norm_inf
from shared_batch_cases import shared_family
from sparse_shared_cases import lasso_path, random_family

K_CLAMP = 13          # 2^-13 .. 2^13: OSQP's [1e-4, 1e4]
RHO, SIGMA, EPS, NUM_ITR_CONV, PASSES = 0.1, 1e-6, 1e-6, 25, 10
NP_DTYPE = {"f64": np.float64, "f32": np.float32}


def _dense(M):
    return M.toarray() if sp.issparse(M) else np.asarray(M, dtype=np.float64)


def _step(v):
    """-floor(e / 2) for v = f 2^e, f in [0.5, 1): the power of two nearest to 1 / sqrt(v) on a log scale; 0 for v = 0."""
    _, e = np.frexp(v)
    return np.where(v > 0, -(e.astype(np.int64) // 2), 0)


def ruiz_pow2(P, A, passes, dtype="f64"):
    """(kd [n], ke [m]) after ``passes`` Jacobi passes; norms in double from the entries rounded to ``dtype`` first."""
    aP = np.abs(_dense(P).astype(NP_DTYPE[dtype]).astype(np.float64))
    aA = np.abs(_dense(A).astype(NP_DTYPE[dtype]).astype(np.float64))
    kd, ke = np.zeros(aP.shape[0], dtype=np.int64), np.zeros(aA.shape[0], dtype=np.int64)
    for _ in range(passes):
        d, e = np.ldexp(1.0, kd), np.ldexp(1.0, ke)
        cn = np.maximum((aP * d[:, None]).max(axis=0) * d, (aA * e[:, None]).max(axis=0) * d)
        rn = (aA * d[None, :]).max(axis=1) * e
        kd = np.clip(kd + _step(cn), -K_CLAMP, K_CLAMP)
        ke = np.clip(ke + _step(rn), -K_CLAMP, K_CLAMP)
    return kd, ke


def scramble(P, A, Q, L, U, spread=1.5, seed=5):
    """Columns by C, rows by R, both 10^U(-spread, spread): P' = C P C, A' = R A C, Q' = Q C, L' = L R, U' = U R (the same QPs in other units)."""
    n, m = P.shape[0], A.shape[0]
    rng = np.random.default_rng(seed)
    C = 10 ** rng.uniform(-spread, spread, n)
    R = 10 ** rng.uniform(-spread, spread, m)
    # P_ij (C_i C_j): C_i C_j is the same double as C_j C_i, so the stored P' is symmetric to the bit (the handles test symmetry with tolerance 0)
    if sp.issparse(P):
        Pc, Ac = sp.coo_matrix(P), sp.coo_matrix(A)
        P2 = sp.csc_matrix((Pc.data * (C[Pc.row] * C[Pc.col]), (Pc.row, Pc.col)), shape=Pc.shape)
        A2 = sp.csc_matrix((Ac.data * (R[Ac.row] * C[Ac.col]), (Ac.row, Ac.col)), shape=Ac.shape)
    else:
        P2, A2 = P * np.outer(C, C), A * np.outer(R, C)
    return P2, A2, Q * C, L * R, U * R


def scrambled_family(n, m, count, spread=1.5, seed=5):
    return scramble(*shared_family(n, m, count), spread=spread, seed=seed)


def scrambled_sparse_family(name, *shape, spread=1.5, seed=5):
    return scramble(*{"lasso": lasso_path, "random": random_family}[name](*shape), spread=spread, seed=seed)


def out_of_range_family():
    """An fp32 family the range check refuses: A[0, 0] = 2e-38 beside 1e4 in its row and its column, P = 1e4 I."""
    n = m = 4
    A = np.eye(m, n)
    A[0, 0], A[0, 1], A[1, 0] = 2e-38, 1e4, 1e4
    return 1e4 * np.eye(n), A, np.ones((2, n)), -np.ones((2, m)), np.ones((2, m))


class EquilibratedRestatement(FamilyRestatement):
    """One family (P, A), the scaling of ``passes`` passes (0: none) and an optional rho scale vS; ``solve`` runs all columns of (Q, L, U) in lock step, under the
    family-wide rho rule when ``adaptive``.  The linear system (both forms) is FamilyRestatement's on the scaled matrices; P0 and A0 are the caller's."""

    def __init__(self, P, A, passes=PASSES, vS=None, *, form, sigma=SIGMA, dtype="f64"):
        self.P0, self.A0 = _dense(P), _dense(A)
        self.kd, self.ke = ruiz_pow2(self.P0, self.A0, passes, dtype)
        self.D, self.E = np.ldexp(1.0, self.kd), np.ldexp(1.0, self.ke)
        super().__init__(self.D[:, None] * self.P0 * self.D[None, :], self.E[:, None] * self.A0 * self.D[None, :], vS, form=form, sigma=sigma)

    def solve(self, Q, L, U, *, X0=None, fctrRho=5.0, rho=RHO, numIterations=5000, epsAbs=EPS, epsRel=EPS, alpha=1.6, numItrConv=NUM_ITR_CONV, adaptive=False):
        Q, L, U = (np.atleast_2d(np.asarray(a, dtype=np.float64)) for a in (Q, L, U))
        count, n, m = Q.shape[0], self.n, self.m
        D, E = self.D[:, None], self.E[:, None]
        X = np.zeros((n, count)) if X0 is None else np.atleast_2d(np.asarray(X0, dtype=np.float64)).T / D       # x~ = D^-1 x
        XP, Z, ZP, Y = np.zeros((n, count)), np.zeros((m, count)), np.zeros((m, count)), np.zeros((m, count))
        Qo = Q.T.copy()
        Qt, Lt, Ut = Qo * D, L.T * E, U.T * E                                                                    # infinite bounds stay infinite
        flags = [ConvergenceFlag.convNumItr] * count
        iters, nref = [numIterations] * count, [0] * count
        rho_col, prop_col = [rho] * count, [rho] * count
        res = [(math.nan, math.nan)] * count
        running = list(range(count))
        rhorho, switches, quotients = rho, [], []
        epsAdmm = min(epsAbs, epsRel) * 1e-2
        self._factorize(rho)
        for ii in range(1, numIterations + 1):
            if not running:
                break
            if adaptive and ((rhorho * fctrRho < rho) or (rhorho > fctrRho * rho)):
                switches.append((ii, rho, rhorho))
                rho = rhorho
                self._factorize(rho)
                for b in running:
                    nref[b] += 1
                    rho_col[b] = rho
            a = np.array(running)
            r, r1 = self.r[:, None], self.r1[:, None]
            XX, ZZ = self._linsys(X[:, a], Qt[:, a], Z[:, a], Y[:, a])
            XP[:, a] = X[:, a]
            X[:, a] = alpha * XX + (1 - alpha) * X[:, a]
            ZP[:, a] = Z[:, a]
            Z[:, a] = _jclamp(alpha * ZZ + (1 - alpha) * Z[:, a] + r1 * Y[:, a], Lt[:, a], Ut[:, a])
            Y[:, a] = Y[:, a] + r * (alpha * ZZ + (1 - alpha) * ZP[:, a] - Z[:, a])
            if ii % numItrConv != 0:
                continue
            norms, stopped = {}, []
            for b in running:
                x, z, y = self.D * X[:, b], Z[:, b] / self.E, self.E * Y[:, b]                                  # the unscaled iterates
                Ax, Px, Aty = self.A0 @ x, self.P0 @ x, self.A0.T @ y
                norms[b] = (_norm_inf(Ax - z), _norm_inf(Px + Qo[:, b] + Aty), _jmax(_norm_inf(Ax), _norm_inf(z)),
                            _jmax(_norm_inf(Px), _norm_inf(Aty), _norm_inf(Qo[:, b])))
                _, flags[b], res[b] = CheckConvergence(x, self.P0, Qo[:, b], self.A0, z, y, self.D * XP[:, b], ZP[:, b] / self.E, 0.0, 0.0, False, epsAbs, epsRel,
                                                       epsAdmm, ConvergenceFlag.convNumItr)
                if flags[b] != ConvergenceFlag.convNumItr:
                    iters[b] = ii
                    stopped.append(b)
            running = [b for b in running if b not in stopped]
            if adaptive:
                rhorho = family_proposal(norms, running, rho, rhorho)
                if running:
                    quotients.append((ii, rhorho / rho))
                for b in running + stopped:
                    prop_col[b] = rhorho
        cols = [dict(x=self.D * X[:, b], z=Z[:, b] / self.E, y=self.E * Y[:, b], convFlag=int(flags[b]), iterations=iters[b], numRefactor=nref[b],
                     rhoFinal=rho_col[b], rhoProposed=prop_col[b], resPrim=res[b][0], resDual=res[b][1]) for b in range(count)]
        return dict(columns=cols, switches=switches, quotients=quotients, rho=rho)


def warm_start(Q):
    """A non-zero, reproducible warm start of the shape of Q, scaled like a solution of the scrambled families (|x| ~ 1 / C)."""
    rng = np.random.default_rng(11)
    return 0.1 * rng.standard_normal(Q.shape)


_FAMILIES, _RUNS = {}, {}


def family(name, *shape):
    """("scrambled", n, m, count[, spread]) | ("plain", n, m, count) | ("lasso" | "random", ...): scrambled sparse families.  Computed once, never changed."""
    key = (name,) + shape
    if key not in _FAMILIES:
        if name == "scrambled":
            _FAMILIES[key] = scrambled_family(*shape)
        elif name == "plain":
            _FAMILIES[key] = shared_family(*shape)
        else:
            _FAMILIES[key] = scrambled_sparse_family(name, *shape)
    return _FAMILIES[key]


def run(key, form, *, passes=PASSES, kind=None, warm=False, dtype="f64", **kw):
    """The restatement's run of family ``key``, computed once per option set and shared by the tests.  kind: None | "equality" (equality_rho_scale)."""
    k = (key, form, passes, kind, warm, dtype, tuple(sorted(kw.items())))
    if k not in _RUNS:
        from quadraticprogramsolver_amd import equality_rho_scale
        P, A, Q, L, U = family(*key)
        vS = equality_rho_scale(L, U) if kind == "equality" else None
        _RUNS[k] = EquilibratedRestatement(P, A, passes, vS, form=form, dtype=dtype).solve(Q, L, U, X0=warm_start(Q) if warm else None, **kw)
    return _RUNS[k]
