"""The per-column adaptive rho of the matrix-free CG shared-matrix batch (qps_set_shared_column_rho) restated in numpy, and the case table of its tests.  Plain
importable helper, no device needed: tests/test_column_rho_cpu.py guards it, tests/test_gpu_column_rho.py and tests/tools/gpu_column_rho_timing.py compare the
device with it.

The loop is the batch loop of family_rho_cases.FamilyRestatement with rho per column: column b runs SolveQuadraticProgram.jl:45-71 on its own rho_b (row i on
rho_b s_i when a scale is given) with the dense KKT or the reduced solve as its linear system, starts from rho_b = rhorho_b = rho (:43), takes
    rhorho_b = clamp(rho_b sqrt((normResPrim_b maxNormDual_b) / (normResDual_b maxNormPrim_b)), 1e-3, 1e6)           (:92-96, its own four norms)
at every check, its stopping check included, and at the top of the next iteration rhorho_b fctrRho < rho_b || rhorho_b > fctrRho rho_b (:47) makes
rho_b = rhorho_b.  The columns do not see each other, so the restatement runs them one after the other.

Beside the result it records, per column, how close every decision came to going the other way: the margin of every :47 decision,
min(|q / f - 1|, |q f - 1|) with q = rhorho_b / rho_b, and the margin of the stopping decision (:102-107) at every check.  A GPU test compares a column only
where those margins say that two correct linear-system paths must take the same decisions."""
import functools
import math

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp

from cg_shared_cases import banded_family
from oracle.qps_oracle_np import ConvergenceFlag, _jclamp, _jmax, _norm_inf
from quadraticprogramsolver_amd import equality_rho_scale
from sparse_shared_cases import random_family

EPS, NUM_ITR_CONV, COUNT = 1e-6, 25, 20
NEVER = 1e12                    # fctrRho at which no proposal inside [1e-3, 1e6] passes :47 from a rho inside it
SWITCH_CLEAR, STOP_CLEAR = 0.02, 0.01      # a column is compared when every :47 decision is 2 % and every stopping decision 1 % clear
FP32_CLEAR = 0.10
EPS32, FP32_TERMS = 2.0 ** -24, 4    # half an ulp of fp32; the terms of one residual entry (a row of A or P with three entries, and the vector it is compared with)
MAX_LEFT_OUT = 2
FLOOR = (1e-7, 1e-7, 1e-6)      # the fixed-rho bounds of tests/test_gpu_cg_shared_batch.py for x, z, y

FAMILIES = {"banded": banded_family, "random": random_family}

# family, start rho, fctrRho, and what tests/test_column_rho_cpu.py measured on the CPU between the C oracle's matrix-free CG (epsPcg 1e-13, 5000 CG iterations)
# and its sparse L D L' over the compared columns, rounded up: the relative spread of rhoFinal and of x, z, y (max |a - b| / max(1, max |b|)).  Two correct
# linear-system paths differ by that much -- the CG stops at sqrt(eps) ||r0|| and the proposal amplifies it -- so the device is held to 10 x the spread (another
# summation order), with FLOOR under x, z, y.  The guard re-measures every figure and fails when one is above twice its row (the figures are rounding noise and
# move with the thread count of the oracle's sums) and above 1e-12, under which the bounds are the floors anyway.
#   measured, to eps = 1e-6: banded20-f5 rho 4.9e-06 x 9.5e-11 z 7.2e-11 y 7.8e-08; random20-f3 rho 1.0e-07 x 1.1e-13 z 2.6e-13 y 1.1e-13
#   measured, K = 100, eps = 0: banded20-f5 rho 2.3e-07 x 2.2e-10 z 1.7e-10 y 1.5e-08; random20-f3 rho 1.8e-07 x 3.8e-14 z 3.2e-14 y 2.0e-14
# (column 9 of the banded and column 6 of the random case are left out: a :47 decision within 0.9 % of a threshold)
CASES = {
    "banded20-f5": dict(family=("banded", COUNT), rho=1.0, fctrRho=5.0, spread=dict(rho=5e-6, x=1e-10, z=8e-11, y=8e-8),
                        spread_k100=dict(rho=3e-7, x=3e-10, z=2e-10, y=2e-8)),
    "random20-f3": dict(family=("random", COUNT), rho=0.1, fctrRho=3.0, spread=dict(rho=1e-7, x=2e-13, z=3e-13, y=2e-13),
                        spread_k100=dict(rho=2e-7, x=4e-14, z=4e-14, y=3e-14)),
}
FIXED_K = 100
LONG_K, LONG_RHO, LONG_SWITCH, LONG_CLEAR = 30, 0.05, 26, 0.05     # banded_family(3, n=LONG_N): every column switches at iteration 26, at least 5 % clear


def _dense(M):
    return M.toarray() if sp.issparse(M) else np.asarray(M, dtype=np.float64)


def _clear(a, b):
    """How far the comparison of a against the threshold b is from going the other way, relative to b (b = 0: a positive a can never pass)."""
    if b == 0.0:
        return math.inf if a != 0.0 else 0.0
    return abs(a / b - 1.0)


def _both(c1, m1, c2, m2):
    """(value, margin) of c1 && c2: true needs both to hold, false needs one false comparison to hold."""
    if c1 and c2:
        return True, min(m1, m2)
    return False, max(m for c, m in ((c1, m1), (c2, m2)) if not c)


def switch_margin(q, f):
    return min(abs(q / f - 1.0), abs(q * f - 1.0))


def proposal(norms, rho):
    """:92-96 from (normResPrim, normResDual, maxNormPrim, maxNormDual): the expression of family_rho_cases.family_proposal with one running column."""
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.float64(norms[0] * norms[3]) / np.float64(norms[1] * norms[2])
        return float(_jclamp(rho * np.sqrt(ratio), 1e-3, 1e6))


class ColumnRestatement:
    """One family (P, A) and an optional row scale; ``solve`` runs every column of (Q, L, U) under the column rule (``adaptive=False``: fixed rho)."""

    def __init__(self, P, A, vS=None, *, form="kkt", sigma=1e-6):
        self.P, self.A = _dense(P), _dense(A)
        self.n, self.m = self.P.shape[0], self.A.shape[0]
        self.form, self.sigma = form, sigma
        self.s = np.ones(self.m) if vS is None else np.asarray(vS, dtype=np.float64)
        self.PI = self.P + sigma * np.eye(self.n)
        if form not in ("reduced", "kkt"):
            raise ValueError(form)

    def _factorize(self, rho):
        r = rho * self.s
        r1 = 1.0 / r
        if self.form == "reduced":
            return r, r1, sla.cho_factor(self.PI + self.A.T @ (r[:, None] * self.A), lower=True)
        return r, r1, sla.lu_factor(np.block([[self.PI, self.A.T], [self.A, -np.diag(r1)]]))

    def _linsys(self, fac, x, q, z, y):
        r, r1, f = fac
        if self.form == "reduced":
            xx = sla.cho_solve(f, self.sigma * x - q + self.A.T @ (r * z - y))
            return xx, self.A @ xx
        v = sla.lu_solve(f, np.concatenate([self.sigma * x - q, z - r1 * y]))
        return v[:self.n], z + r1 * (v[self.n:] - y)

    def solve_column(self, q, l, u, *, rho, fctrRho, numIterations=5000, epsAbs=EPS, epsRel=EPS, alpha=1.6, numItrConv=NUM_ITR_CONV, adaptive=True,
                     x0=None, z0=None, y0=None):
        n, m = self.n, self.m
        x = np.zeros(n) if x0 is None else np.array(x0, dtype=np.float64)
        z = np.zeros(m) if z0 is None else np.array(z0, dtype=np.float64)
        y = np.zeros(m) if y0 is None else np.array(y0, dtype=np.float64)
        xp, zp = np.zeros(n), np.zeros(m)
        rho = float(rho)
        rhorho, epsAdmm = rho, min(epsAbs, epsRel) * 1e-2
        flag, iters, res = ConvergenceFlag.convNumItr, numIterations, (math.nan, math.nan)
        switches, decisions, stops, checks = [], [], [], []
        fac = self._factorize(rho)
        for ii in range(1, numIterations + 1):
            if adaptive and ii > 1 and (ii - 1) % numItrConv == 0:                            # rhorho moves at a check only: :47 can change its answer there
                with np.errstate(invalid="ignore"):
                    decisions.append((ii, rhorho / rho, switch_margin(rhorho / rho, fctrRho)))
            if adaptive and ((rhorho * fctrRho < rho) or (rhorho > fctrRho * rho)):           # :47
                switches.append((ii, rho, rhorho))
                rho = rhorho
                fac = self._factorize(rho)
            r, r1 = fac[0], fac[1]
            xx, zz = self._linsys(fac, x, q, z, y)
            xp = x
            x = alpha * xx + (1 - alpha) * x                                                  # :56-57
            zp = z
            z = _jclamp(alpha * zz + (1 - alpha) * zp + r1 * y, l, u)                         # :60
            y = y + r * (alpha * zz + (1 - alpha) * zp - z)                                   # :61
            if ii % numItrConv != 0:
                continue
            Ax, Px, Aty = self.A @ x, self.P @ x, self.A.T @ y
            norms = (_norm_inf(Ax - z), _norm_inf(Px + q + Aty), _jmax(_norm_inf(Ax), _norm_inf(z)), _jmax(_norm_inf(Px), _norm_inf(Aty), _norm_inf(q)))
            res = norms[:2]
            checks.append((ii, norms))
            if adaptive:
                rhorho = proposal(norms, rho)                                                 # :92-96
            epsP, epsD = epsAbs + epsRel * norms[2], epsAbs + epsRel * norms[3]               # :99-100
            dx, dz = _norm_inf(x - xp), _norm_inf(z - zp)
            pd, mpd = _both(norms[0] < epsP, _clear(norms[0], epsP), norms[1] < epsD, _clear(norms[1], epsD))          # :102
            ad, mad = _both(dx <= epsAdmm, _clear(dx, epsAdmm), dz <= epsAdmm, _clear(dz, epsAdmm))                    # :105
            stops.append((ii, mad if ad else min(mad, mpd)))                                  # convAdmm wins over convPrimDual
            if pd:
                flag = ConvergenceFlag.convPrimDual
            if ad:
                flag = ConvergenceFlag.convAdmm
            if flag != ConvergenceFlag.convNumItr:
                iters = ii
                break
        return dict(x=x, z=z, y=y, convFlag=int(flag), iterations=iters, numRefactor=len(switches), rhoFinal=rho, rhoProposed=rhorho, resPrim=res[0],
                    resDual=res[1], switches=switches, decisions=decisions, stops=stops, checks=checks)

    def solve(self, Q, L, U, *, X0=None, Z0=None, Y0=None, **kw):
        Q, L, U = (np.atleast_2d(np.asarray(a, dtype=np.float64)) for a in (Q, L, U))
        pick = lambda M, b: None if M is None else M[b]
        return [self.solve_column(Q[b], L[b], U[b], x0=pick(X0, b), z0=pick(Z0, b), y0=pick(Y0, b), **kw) for b in range(Q.shape[0])]


def switch_clearance(col, upto=None):
    """The smallest margin of the column's :47 decisions (those at the top of iterations <= ``upto``); inf when there was none."""
    return min([m for ii, _, m in col["decisions"] if upto is None or ii <= upto], default=math.inf)


def stop_clearance(col):
    """The margin of the stopping decision at the column's last check and the check before it."""
    return min([m for _, m in col["stops"][-2:]], default=math.inf)


def fp32_resolves(col, upto):
    """Whether an fp32 handle can take the column's :47 decisions up to iteration ``upto`` at all.  The check forms A x - z and P x + q + A'y from fp32 panels: an
    entry is a sum of up to FP32_TERMS terms of the size of maxNorm, each rounded once, so a residual norm carries an absolute error of up to
    FP32_TERMS EPS32 maxNorm and the proposal, the square root of a quotient of the two, a relative error of half the sum of the two relative errors.  Two
    exclusions follow, and no more: a decision whose estimated error exceeds its margin is taken on rounding noise; and a proposal that is TAKEN (a switch)
    becomes the rho of every later iteration and decision, so both residual norms behind it have to be resolved at all -- above their own error bound (column
    18 of the banded case switches at iteration 51 on a relative dual residual of 4.5e-8, below EPS32, and then takes one switch where fp64 takes two)."""
    taken = {s[0] for s in col["switches"]}
    for (ii, _, margin), (_, norms) in zip(col["decisions"], col["checks"]):
        if ii > upto:
            break
        with np.errstate(divide="ignore"):
            err = 0.5 * FP32_TERMS * EPS32 * (np.float64(norms[2]) / norms[0] + np.float64(norms[3]) / norms[1])
        if not err <= margin:
            return False
        if ii in taken and not FP32_TERMS * EPS32 * max(np.float64(norms[2]) / norms[0], np.float64(norms[3]) / norms[1]) <= 1.0:
            return False
    return True


def compared_fp32(cols, upto):
    """The columns an fp32 run is compared on: every :47 decision up to ``upto`` FP32_CLEAR clear of its thresholds and resolved by the format."""
    return [b for b in compared(cols, switch_clear=FP32_CLEAR, stop_clear=0.0, upto=upto) if fp32_resolves(cols[b], upto)]


def compared(cols, *, switch_clear=SWITCH_CLEAR, stop_clear=STOP_CLEAR, upto=None):
    """The columns whose decisions are all clear of their thresholds: those a test may hold to equal flags, iterations and switch counts."""
    return [b for b, c in enumerate(cols) if switch_clearance(c, upto) >= switch_clear and stop_clearance(c) >= stop_clear]


def equality_scale(L, U):
    """The scale of the composition row: 1e3 on the rows that are equalities in column 2 (no row is one in every column, which is what equality_rho_scale of
    the whole family asks for), 1 elsewhere; shared by all columns like every scale."""
    vS = equality_rho_scale(L[2], U[2])
    assert 0 < np.count_nonzero(vS != 1.0) < vS.size
    return vS


def case_data(name):
    c = CASES[name]
    return FAMILIES[c["family"][0]](*c["family"][1:])


@functools.lru_cache(maxsize=None)
def case_run(name, form="kkt", fixed_k=None, fctrRho=None, scale=None):
    """The restatement's run of a case, computed once per (case, options) and shared by the tests; nobody changes what it returns.  ``fixed_k``: that many
    iterations with eps = 0.  ``scale`` = "equality": equality_scale of the family."""
    c = CASES[name]
    P, A, Q, L, U = case_data(name)
    kw = dict(rho=c["rho"], fctrRho=c["fctrRho"] if fctrRho is None else fctrRho)
    if fixed_k:
        kw.update(numIterations=fixed_k, epsAbs=0.0, epsRel=0.0)
    vS = equality_scale(L, U) if scale == "equality" else None
    return ColumnRestatement(P, A, vS, form=form).solve(Q, L, U, **kw)


def tolerances(name, fixed_k=False):
    """(rhoFinal, x, z, y) bounds of the device against the C oracle on a case: 10 x the recorded spread, FLOOR under x, z, y."""
    s = CASES[name]["spread_k100" if fixed_k else "spread"]
    return 10 * s["rho"], max(10 * s["x"], FLOOR[0]), max(10 * s["z"], FLOOR[1]), max(10 * s["y"], FLOOR[2])


@functools.lru_cache(maxsize=None)
def oracle_run(name, kind="cg", fixed_k=None):
    """The C oracle's solve of every column of a case with adptRho: ``kind`` "cg" = KIND_CG_MATFREE at epsPcg 1e-13 and 5000 CG iterations, "ldl" =
    KIND_KKT_LDL_SPARSE.  A list of (x, info) per column, computed once and shared; nobody changes what it returns."""
    from oracle import c_oracle as co
    c = CASES[name]
    P, A, Q, L, U = case_data(name)
    kw = dict(rho=c["rho"], fctrRho=c["fctrRho"], adptRho=True, numItrConv=NUM_ITR_CONV)
    kw.update(dict(linsys=co.KIND_CG_MATFREE, epsPcg=1e-13, numItrPcg=5000) if kind == "cg" else dict(linsys=co.KIND_KKT_LDL_SPARSE))
    kw.update(dict(numIterations=fixed_k, epsAbs=0.0, epsRel=0.0) if fixed_k else dict(numIterations=5000, epsAbs=EPS, epsRel=EPS))
    perm = co.kkt_ordering(P, A) if kind == "ldl" else None
    return [co.solve(P, Q[b], A, L[b], U[b], perm=perm, **kw) for b in range(Q.shape[0])]


# ---- the rows of the composition tests: the device against the restatement itself ------------------------------------------------------------------------
# Both run the banded case for FIXED_K iterations with eps = 0.  "equality": equality_scale (1e3 on the equality rows of column 2) on top of the column rule.
# "warm": a second solve in warm start mode "state" after update(mQ = warm_q(Q)), from the x, z, y the first left behind and from rho = the start rho again.
# spread: how far the reduced and the KKT form of the restatement disagree among themselves over the compared columns, measured by the guard and rounded up
# (equality: rho 2.1e-11 x 4.7e-13 z 3.7e-13 y 1.9e-11; warm: rho 2.4e-08 x 4.0e-13 z 3.7e-13 y 3.6e-11); the device is held to 10 x that, FLOOR under x, z, y
# and the 10 x rho spread of the case's own K = 100 row under rhoFinal: the device's CG is one more path, as far from either form as the oracle's CG.
EQUALITY_FCTR = 3.0             # at fctrRho = 5 column 2 itself proposes 5.056 rho at iteration 25, 1.1 % from the threshold; at 3 all 20 columns are clear
COMPOSE = {"equality": dict(rho=3e-11, x=5e-13, z=4e-13, y=2e-11), "warm": dict(rho=3e-8, x=4e-13, z=4e-13, y=4e-11)}


def warm_q(Q):
    return Q + 0.05 * np.roll(Q, 1, axis=0)


@functools.lru_cache(maxsize=None)
def compose_run(kind, form="kkt"):
    """The restatement's columns of a composition row (for "warm": of the second solve)."""
    name = "banded20-f5"
    if kind == "equality":
        return case_run(name, form=form, fixed_k=FIXED_K, scale="equality", fctrRho=EQUALITY_FCTR)
    c = CASES[name]
    P, A, Q, L, U = case_data(name)
    first = case_run(name, form=form, fixed_k=FIXED_K)
    X0, Z0, Y0 = (np.array([k[v] for k in first]) for v in "xzy")
    return ColumnRestatement(P, A, form=form).solve(warm_q(Q), L, U, X0=X0, Z0=Z0, Y0=Y0, rho=c["rho"], fctrRho=c["fctrRho"], numIterations=FIXED_K, epsAbs=0.0,
                                                    epsRel=0.0)


def compose_tolerances(kind):
    s, base = COMPOSE[kind], CASES["banded20-f5"]["spread_k100"]
    return max(10 * s["rho"], 10 * base["rho"]), max(10 * s["x"], FLOOR[0]), max(10 * s["z"], FLOOR[1]), max(10 * s["y"], FLOOR[2])


# banded_family(3, n=LONG_N) at K = LONG_K: the spread of the oracle's CG against its sparse L D L' (measured rho 3.8e-08 x 1.0e-08 z 1.4e-08 y 7.1e-09)
LONG_SPREAD = dict(rho=4e-8, x=1e-8, z=2e-8, y=8e-9)


def long_tolerances():
    s = LONG_SPREAD
    return 10 * s["rho"], max(10 * s["x"], FLOOR[0]), max(10 * s["z"], FLOOR[1]), max(10 * s["y"], FLOOR[2])
