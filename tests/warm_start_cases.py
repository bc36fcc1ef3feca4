"""The opt-in warm start of z and y of the shared-matrix batches (qps_set_shared_warm_start, qps_set_shared_dual) restated in numpy, the perturbation of its
re-solve sequences and their case table.  Plain importable helper, no device needed: tests/test_warm_start_cpu.py guards it, tests/test_gpu_warm_start.py and
tests/tools/gpu_warm_start_timing.py compare the device with it.

``WarmRestatement.solve_from`` is the batch loop of tests/family_rho_cases.py (``FamilyRestatement``) with the state passed in.  It derives from
``EquilibratedRestatement`` of tests/equilibration_cases.py -- itself a ``FamilyRestatement`` -- so that one loop serves the handles with and without scaling:
``passes = 0`` makes D = E = 1 and every product with them exact, i.e. the loop of ``FamilyRestatement`` bit for bit.  State goes in and comes out in the caller's
units (x~ = D^-1 x, z~ = E z, y~ = E^-1 y inside).  Mode 1 of the handles is ``solve_from(Q, L, U, X0, Z0, Y0)``, mode 2 is ``Z0 = X0 @ A.T``; xp and zp restart
at 0 and the iteration counter at 1, as on the device."""
import math

import numpy as np

from equilibration_cases import EPS, NUM_ITR_CONV, RHO, EquilibratedRestatement, _dense
from family_rho_cases import family_proposal
from oracle.qps_oracle_np import ConvergenceFlag, _jclamp, _jmax, _norm_inf
from shared_batch_cases import shared_family
from sparse_shared_cases import lasso_path, random_family

FAMILIES = {"shared": shared_family, "lasso": lasso_path, "random": random_family}
STEPS = 3

# Re-solve sequences at rho = 0.1, eps = 1e-6, numItrConv = 25: a cold solve of the family, then for k = 1..STEPS the data ``step(Q, L, U, k)`` solved from the
# state the solve before left (x, z, y of every column's own stopping iteration).  Per solve and column: the stopping iteration and the flag the CPU run of both
# forms gives.  "x_only": the same data solved from the x of the solve before and z = y = 0 (what the handles do in mode 0) -- the comparison the timing tool
# prints, never asserted on a device.  ``form``: the restatement the handle of the GPU test is compared with (dense handle: reduced, sparse handle: kkt).
# tests/test_warm_start_cpu.py holds every row to these figures, in both forms, and to its rounding guard.
_R20 = [200, 75, 75, 100, 50, 50, 100, 50, 75, 50, 75, 50, 50, 75, 75, 50, 75, 50, 50, 50]
CASES = {
    "shared96": dict(family=("shared", 96, 160, 4), form="reduced",
                     iterations=[[3575, 475, 450, 325], [1225, 400, 425, 225], [1825, 400, 500, 225], [2150, 325, 475, 225]], flags=[[3] * 4] * 4,
                     x_only=[[3575, 475, 450, 325], [1750, 450, 475, 325], [3075, 475, 525, 325], [3275, 425, 425, 325]]),
    "shared200": dict(family=("shared", 200, 330, 4), form="reduced",
                      iterations=[[1975, 350, 400, 250], [1275, 225, 325, 200], [1675, 225, 300, 175], [1900, 275, 300, 200]], flags=[[3] * 4] * 4,
                      x_only=[[1975, 350, 400, 250], [1525, 300, 400, 250], [2400, 325, 375, 250], [1900, 350, 375, 275]]),
    "random20": dict(family=("random", 20), form="kkt",
                     iterations=[_R20,
                                 [175, 50, 75, 50, 50, 50, 75, 50, 50, 50, 50, 25, 50, 75, 50, 50, 75, 50, 50, 25],
                                 [150, 75, 75, 75, 50, 50, 75, 50, 50, 50, 50, 50, 50, 75, 75, 50, 75, 50, 50, 25],
                                 [175, 75, 75, 50, 50, 50, 50, 50, 50, 50, 50, 50, 50, 75, 75, 50, 75, 50, 50, 50]],
                     flags=[[3] * 20, [3] * 4 + [2] + [3] * 15, [3] * 5 + [2] + [3] * 5 + [2] + [3] * 8, [3] * 5 + [2] + [3] * 5 + [2] + [3] * 5 + [2] + [3] * 2],
                     x_only=[_R20, _R20,
                             [200, 75, 75, 100, 50, 50, 75, 50, 75, 75, 75, 50, 50, 75, 100, 50, 75, 50, 50, 50],
                             [200, 75, 75, 100, 50, 50, 75, 50, 75, 50, 75, 50, 50, 75, 75, 50, 75, 50, 50, 50]]),
}


def step(Q, L, U, k, pert=0.02, seed=11):
    """Deterministic perturbation number k of (Q, L, U): q moves by pert mean|Q| randn, l and u move together by pert randn (infinite bounds stay infinite)."""
    rng = np.random.default_rng([seed, k])
    Q2 = Q + pert * np.mean(np.abs(Q)) * rng.standard_normal(Q.shape)
    d = pert * rng.standard_normal(L.shape)
    return Q2, L + d, U + d


class WarmRestatement(EquilibratedRestatement):
    """One family (P, A), the scaling of ``passes`` passes (0, the default here: none) and an optional rho scale vS."""

    def __init__(self, P, A, passes=0, vS=None, *, form, **kw):
        super().__init__(P, A, passes, vS, form=form, **kw)

    def solve_from(self, Q, L, U, X0=None, Z0=None, Y0=None, *, fctrRho=5.0, rho=RHO, numIterations=5000, epsAbs=EPS, epsRel=EPS, alpha=1.6,
                   numItrConv=NUM_ITR_CONV, adaptive=False):
        """X0 [count x n], Z0, Y0 [count x m] in the caller's units (None: zeros).  Returns the dict of ``solve`` plus X, Z, Y ([count x .], the caller's units)
        and ``trace``: per column the list of (iteration, (resPrim / epsPrim, resDual / epsDual, |dx| / epsAdmm, |dz| / epsAdmm)) of every check it ran."""
        Q, L, U = (np.atleast_2d(np.asarray(a, dtype=np.float64)) for a in (Q, L, U))
        count, n, m = Q.shape[0], self.n, self.m
        D, E = self.D[:, None], self.E[:, None]
        start = lambda V, rows: np.zeros((rows, count)) if V is None else np.atleast_2d(np.asarray(V, dtype=np.float64)).T.copy()
        X, Z, Y = start(X0, n) / D, start(Z0, m) * E, start(Y0, m) / E
        XP, ZP = np.zeros((n, count)), np.zeros((m, count))
        Qo = Q.T.copy()
        Qt, Lt, Ut = Qo * D, L.T * E, U.T * E
        flags = [ConvergenceFlag.convNumItr] * count
        iters, nref = [numIterations] * count, [0] * count
        rho_col, prop_col = [rho] * count, [rho] * count
        res = [(math.nan, math.nan)] * count
        running = list(range(count))
        rhorho, switches, quotients = rho, [], []
        trace = [[] for _ in range(count)]
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
                dx, dz = _norm_inf(x - self.D * XP[:, b]), _norm_inf(z - ZP[:, b] / self.E)
                epsPrim, epsDual = epsAbs + epsRel * norms[b][2], epsAbs + epsRel * norms[b][3]                 # SolveQuadraticProgram.jl:99-100
                if (norms[b][0] < epsPrim) and (norms[b][1] < epsDual):                                         # :102-104
                    flags[b] = ConvergenceFlag.convPrimDual
                if (dx <= epsAdmm) and (dz <= epsAdmm):                                                         # :105-107 (not else)
                    flags[b] = ConvergenceFlag.convAdmm
                res[b] = (norms[b][0], norms[b][1])
                with np.errstate(divide="ignore", invalid="ignore"):
                    trace[b].append((ii, tuple(float(np.float64(p) / np.float64(q)) for p, q in
                                               ((norms[b][0], epsPrim), (norms[b][1], epsDual), (dx, epsAdmm), (dz, epsAdmm)))))
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
        Xo, Zo, Yo = (X * D).T.copy(), (Z / E).T.copy(), (Y * E).T.copy()
        cols = [dict(x=Xo[b], z=Zo[b], y=Yo[b], convFlag=int(flags[b]), iterations=iters[b], numRefactor=nref[b], rhoFinal=rho_col[b], rhoProposed=prop_col[b],
                     resPrim=res[b][0], resDual=res[b][1]) for b in range(count)]
        return dict(columns=cols, switches=switches, quotients=quotients, rho=rho, X=Xo, Z=Zo, Y=Yo, trace=trace)


_FAMILIES, _DATA, _RUNS = {}, {}, {}


def family(name, *shape):
    """The family of a key such as ("shared", 96, 160, 4), computed once and never changed."""
    key = (name,) + shape
    if key not in _FAMILIES:
        _FAMILIES[key] = FAMILIES[name](*shape)
    return _FAMILIES[key]


def sequence_data(name):
    """[(Q, L, U)] of the cold solve and of the STEPS perturbed re-solves of a row of CASES (step k perturbs the family's own data: the sequence stays near it)."""
    if name not in _DATA:
        _, _, Q, L, U = family(*CASES[name]["family"])
        _DATA[name] = [(Q, L, U)] + [step(Q, L, U, k) for k in range(1, STEPS + 1)]
    return _DATA[name]


def sequence_run(name, form, warm=True):
    """The restatement's runs of a row of CASES in ``form``: the cold solve, then every step from the state of the run before (``warm=False``: from its x alone,
    z = y = 0).  Computed once and shared by the tests; nobody changes what it returns."""
    key = (name, form, warm)
    if key not in _RUNS:
        P, A = family(*CASES[name]["family"])[:2]
        R = WarmRestatement(P, A, form=form)
        runs = []
        for Q, L, U in sequence_data(name):
            if not runs:
                runs.append(R.solve_from(Q, L, U))
            elif warm:
                runs.append(R.solve_from(Q, L, U, runs[-1]["X"], runs[-1]["Z"], runs[-1]["Y"]))
            else:
                runs.append(R.solve_from(Q, L, U, runs[-1]["X"]))
        _RUNS[key] = runs
    return _RUNS[key]


def dense(M):
    return _dense(M)
