"""The family-wide adaptive rho of the shared-matrix batches (qps_set_shared_adaptive_rho) restated in numpy, and the case table of its tests.  Plain importable
helper, no device needed: tests/test_family_rho_cpu.py guards it, tests/test_gpu_family_rho.py and tests/tools/gpu_family_rho_timing.py compare the device with it.

The loop is the batch loop of the handles: every column runs SolveQuadraticProgram.jl:54-61 on ONE rho (row i on rho s_i when a scale is given), in the reduced
Cholesky form (dense handle) or the dense KKT form (sparse handle) of tests/rho_scale_cases.py; every column has its own check (:79-112) and is frozen once it
stops.  The rule, at a check and after the per-column decisions: over the columns still running, bp = argmax normResPrim / maxNormPrim and bd = argmax
normResDual / maxNormDual (lowest index on ties, a NaN quotient never wins against a number),
    rhorho = clamp(rho sqrt((normResPrim_bp maxNormDual_bd) / (normResDual_bd maxNormPrim_bp)), 1e-3, 1e6)           (:92-96 on the worst columns)
and at the top of the next iteration rhorho fctrRho < rho || rhorho > fctrRho rho (:47) makes rho = rhorho with one re-factorisation for all columns."""
import math

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp

from oracle.qps_oracle_np import CheckConvergence, ConvergenceFlag, _jclamp, _jmax, _norm_inf
from quadraticprogramsolver_amd import equality_rho_scale
from rho_scale_cases import scale_of
from shared_batch_cases import shared_family
from sparse_shared_cases import lasso_path, random_family

RHO, EPS, NUM_ITR_CONV = 0.1, 1e-6, 25
FAMILIES = {"shared": shared_family, "lasso": lasso_path, "random": random_family}

# family, scale kind (None: scalar rho), fctrRho, and what the CPU run of both forms gives at rho = 0.1, eps = 1e-6, numItrConv = 25: the iterations at whose top
# rho switched, and per column the stopping iteration and the flag.  tests/test_family_rho_cpu.py holds every row to these figures and to its rounding guard.
# rho_spread: how far the reduced and the KKT form of the restatement disagree among themselves, relatively, in the rho of a switch (the largest over the switches,
# rounded up; measured 1.5e-9, 5.9e-6 and 2.8e-9 on the three rows that name it).  Rows without it are held to 1e-11, a tenth of the 1e-10 the device is held to.
CASES = {
    "shared96-f5": dict(family=("shared", 96, 160, 4), kind=None, fctrRho=5.0, switches=[26], iterations=[525, 75, 100, 100], flags=[3, 3, 3, 3]),
    "shared96-f3": dict(family=("shared", 96, 160, 4), kind=None, fctrRho=3.0, switches=[26, 101], iterations=[225, 75, 100, 100], flags=[3, 3, 3, 3]),
    "shared96-eq-f5": dict(family=("shared", 96, 160, 4), kind="equality", fctrRho=5.0, switches=[26], iterations=[325, 75, 75, 100], flags=[3, 3, 3, 3]),
    "shared200-f5": dict(family=("shared", 200, 330, 4), kind=None, fctrRho=5.0, switches=[26], iterations=[425, 100, 100, 75], flags=[3, 3, 3, 3]),
    "lasso10-f4": dict(family=("lasso", 10, 6), kind=None, fctrRho=4.0, switches=[26, 76, 126, 176], iterations=[150, 175, 200, 200, 200, 200],
                       flags=[3, 3, 2, 2, 2, 2], rho_spread=2e-9),
    "shared200-eq-f5": dict(family=("shared", 200, 330, 4), kind="equality", fctrRho=5.0, switches=[26], iterations=[275, 100, 75, 100], flags=[3, 3, 3, 3]),
    # fixed K, eps = 0 (no column stops): the fp32 case, and the shape of tests/test_gpu_shared_batch.py that runs the staged kernel form on three panels -- with
    # the equality scale at factor 10: at factor 1e3 the two forms of the restatement already disagree by 9e-11 in the rho of the first switch at this size
    "shared96-f5-k100": dict(family=("shared", 96, 160, 4), kind=None, fctrRho=5.0, fixed_k=100, switches=[26], iterations=[100] * 4, flags=[1] * 4),
    "shared2112-eq10-f5-k60": dict(family=("shared", 2112, 2304, 37), kind="equality10", fctrRho=5.0, fixed_k=60, switches=[26], iterations=[60] * 37, flags=[1] * 37),
    # the same shape to eps = 1e-6 with numIterations = 175: fifteen columns stop on their own between iterations 75 and 175, the others end with flag 1.  Left to
    # run on, rho switches again at iteration 176 (200, with the equality scale 76 / 101 and 176), and there the two forms of the restatement disagree among
    # themselves by 3e-8 to 3e-6 in the new rho: no reference for a 1e-10 comparison, so those runs are not in the table (rho_spread below)
    "shared2112-f5-n175": dict(family=("shared", 2112, 2304, 37), kind=None, fctrRho=5.0, num_iterations=175, switches=[26],
                               iterations=[175, 100, 75, 100, 100, 125, 125, 150, 175, 150, 150] + [175] * 26, flags=[3] * 15 + [1] * 22),
    "lasso10-eq-f4": dict(family=("lasso", 10, 6), kind="equality", fctrRho=4.0, switches=[26, 76, 151, 201], iterations=[175, 175, 200, 200, 200, 225],
                          flags=[3, 3, 3, 3, 3, 2], rho_spread=6e-6),
    "random20-f5": dict(family=("random", 20), kind=None, fctrRho=5.0, switches=[51, 101],
                        iterations=[100, 100, 75, 75, 50, 50, 100, 50, 75, 50, 75, 50, 50, 125, 125, 50, 125, 50, 50, 50], flags=[2] + [3] * 19, rho_spread=3e-9),
    # the pattern scale to eps = 1e-6 takes thousands of iterations on every family tried and its quotients pass within 0.3 % of fctrRho; at a fixed K = 175 the one
    # switch (rho goes DOWN, 0.1 -> 0.018 at iteration 151) is 9 % clear
    "random20-pat-f5-k175": dict(family=("random", 20), kind="pattern", fctrRho=5.0, fixed_k=175, switches=[151], iterations=[175] * 20, flags=[1] * 20),
}


def _dense(M):
    return M.toarray() if sp.issparse(M) else np.asarray(M, dtype=np.float64)


def _quotient(a, b):
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.float64(a) / np.float64(b))


def _argmax_no_nan(vals, running):
    """Lowest index of the largest value among ``running``; a NaN only when every value is NaN."""
    best = -1
    for b in running:
        if best < 0 or (math.isnan(vals[best]) and not math.isnan(vals[b])) or vals[b] > vals[best]:
            best = b
    return best


def family_proposal(norms, running, rho, rhorho):
    """norms[b] = (normResPrim, normResDual, maxNormPrim, maxNormDual) of column b; the proposal from the columns of ``running`` (none: rhorho stays)."""
    if not running:
        return rhorho
    qp = {b: _quotient(norms[b][0], norms[b][2]) for b in running}
    qd = {b: _quotient(norms[b][1], norms[b][3]) for b in running}
    bp, bd = _argmax_no_nan(qp, running), _argmax_no_nan(qd, running)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.float64(norms[bp][0] * norms[bd][3]) / np.float64(norms[bd][1] * norms[bp][2])
        return float(_jclamp(rho * np.sqrt(ratio), 1e-3, 1e6))


class FamilyRestatement:
    """One family (P, A) and an optional scale; ``solve`` runs all columns of (Q, L, U) in lock step under the family rule (``adaptive=False``: fixed rho)."""

    def __init__(self, P, A, vS=None, *, form, sigma=1e-6):
        self.P, self.A = _dense(P), _dense(A)
        self.n, self.m = self.P.shape[0], self.A.shape[0]
        self.form, self.sigma = form, sigma
        self.s = np.ones(self.m) if vS is None else np.asarray(vS, dtype=np.float64)
        self.PI = self.P + sigma * np.eye(self.n)
        if form not in ("reduced", "kkt"):
            raise ValueError(form)

    def _factorize(self, rho):
        self.r = rho * self.s
        self.r1 = 1.0 / self.r
        if self.form == "reduced":
            self.fac = sla.cho_factor(self.PI + self.A.T @ (self.r[:, None] * self.A), lower=True)
        else:
            self.fac = sla.lu_factor(np.block([[self.PI, self.A.T], [self.A, -np.diag(self.r1)]]))

    def _linsys(self, X, Q, Z, Y):
        """Columns side by side: X, Q are n x k, Z, Y are m x k."""
        r, r1 = self.r[:, None], self.r1[:, None]
        if self.form == "reduced":
            XX = sla.cho_solve(self.fac, self.sigma * X - Q + self.A.T @ (r * Z - Y))
            return XX, self.A @ XX
        V = sla.lu_solve(self.fac, np.vstack([self.sigma * X - Q, Z - r1 * Y]))
        return V[:self.n], Z + r1 * (V[self.n:] - Y)

    def solve(self, Q, L, U, *, fctrRho=5.0, rho=RHO, numIterations=5000, epsAbs=EPS, epsRel=EPS, alpha=1.6, numItrConv=NUM_ITR_CONV, adaptive=True):
        Q, L, U = (np.atleast_2d(np.asarray(a, dtype=np.float64)) for a in (Q, L, U))
        count, n, m = Q.shape[0], self.n, self.m
        X, XP = np.zeros((n, count)), np.zeros((n, count))
        Z, ZP, Y = np.zeros((m, count)), np.zeros((m, count)), np.zeros((m, count))
        Qt, Lt, Ut = Q.T.copy(), L.T.copy(), U.T.copy()
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
            if adaptive and ((rhorho * fctrRho < rho) or (rhorho > fctrRho * rho)):          # :47
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
            X[:, a] = alpha * XX + (1 - alpha) * X[:, a]                                      # :56-57
            ZP[:, a] = Z[:, a]
            Z[:, a] = _jclamp(alpha * ZZ + (1 - alpha) * Z[:, a] + r1 * Y[:, a], Lt[:, a], Ut[:, a])   # :60
            Y[:, a] = Y[:, a] + r * (alpha * ZZ + (1 - alpha) * ZP[:, a] - Z[:, a])           # :61
            if ii % numItrConv != 0:
                continue
            norms, stopped = {}, []
            for b in running:
                x, z, y = X[:, b], Z[:, b], Y[:, b]
                Ax, Px, Aty = self.A @ x, self.P @ x, self.A.T @ y
                norms[b] = (_norm_inf(Ax - z), _norm_inf(Px + Qt[:, b] + Aty), _jmax(_norm_inf(Ax), _norm_inf(z)),
                            _jmax(_norm_inf(Px), _norm_inf(Aty), _norm_inf(Qt[:, b])))
                _, flags[b], res[b] = CheckConvergence(x, self.P, Qt[:, b], self.A, z, y, XP[:, b], ZP[:, b], 0.0, 0.0, False, epsAbs, epsRel, epsAdmm,
                                                       ConvergenceFlag.convNumItr)
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
        cols = [dict(x=X[:, b].copy(), z=Z[:, b].copy(), y=Y[:, b].copy(), convFlag=int(flags[b]), iterations=iters[b], numRefactor=nref[b],
                     rhoFinal=rho_col[b], rhoProposed=prop_col[b], resPrim=res[b][0], resDual=res[b][1]) for b in range(count)]
        return dict(columns=cols, switches=switches, quotients=quotients, rho=rho)


def case_data(name):
    """(P, A, Q, L, U, scale or None, fctrRho) of a row of CASES.  Kind "equality10": the equality scale with factor 10 instead of 1e3."""
    c = CASES[name]
    P, A, Q, L, U = FAMILIES[c["family"][0]](*c["family"][1:])
    if c["kind"] == "equality10":
        return P, A, Q, L, U, equality_rho_scale(L, U, factor=10.0), c["fctrRho"]
    return P, A, Q, L, U, (None if c["kind"] is None else scale_of(c["kind"], L, U)), c["fctrRho"]


_RUNS = {}


def case_run(name, form, **kw):
    """The restatement's run of a case, computed once per (case, form, options) and shared by the tests; nobody changes what it returns.  A case with ``fixed_k``
    runs that many iterations with eps = 0, one with ``num_iterations`` runs to eps = 1e-6 or that many iterations."""
    if "fixed_k" in CASES[name]:
        kw = dict(dict(numIterations=CASES[name]["fixed_k"], epsAbs=0.0, epsRel=0.0), **kw)
    if "num_iterations" in CASES[name]:
        kw = dict(dict(numIterations=CASES[name]["num_iterations"]), **kw)
    key = (name, form, tuple(sorted(kw.items())))
    if key not in _RUNS:
        P, A, Q, L, U, s, f = case_data(name)
        _RUNS[key] = FamilyRestatement(P, A, s, form=form).solve(Q, L, U, fctrRho=f, **kw)
    return _RUNS[key]
