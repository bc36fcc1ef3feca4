"""Host-side mirror of the reference interface for the ADMM QP path, driving libqps_hip.so through its C ABI.

Reference (file:line under RoyiAvital/QuadraticProgramSolver):
  SolveQuadraticProgram!(vX, mP, vQ, mA, vL, vU, LinSysSolInit, LinSysSol!; kw...)   SolveQuadraticProgram.jl:14-76
  @enum LinearSolverMode / ConvergenceFlag                                          SolveQuadraticProgram.jl:11-12
  plugin pair Init / Sol!                                                            LinearSystemSolvers.jl:16-229

Python cannot spell ``!`` in an identifier, so the mutating function is ``SolveQuadraticProgramInplace`` (alias
``SolveQuadraticProgram_b``); positional order, keyword names (including the Unicode ones) and the returned enum are
the reference's.  The Julia ``ccall`` wrapper that keeps the exact spelling lives in julia/QuadraticProgramSolverHIP.jl.

Passing the sentinel pair ``(HipCholInit, HipChol)`` (dense reduced-form Cholesky) or ``(HipCgInit, HipCg)`` (CSR
matrix-free CG) routes the whole loop to the device-resident implementation.  The pairs are also callable literally
with the reference plugin signature (host vectors in, device solve, host vectors out) so that an unmodified
reference-style loop can drive the GPU linear solve.  There is no CPU implementation in this package.
"""
from __future__ import annotations

import ctypes as C
import enum

import numpy as np
import scipy.sparse as sp

from . import _lib
from ._lib import QPS_F32, QPS_F64, QPS_LINSYS_AUTO, QPS_LINSYS_CG, QPS_LINSYS_CG_EXPLICIT, QPS_LINSYS_CHOLESKY, QPS_LINSYS_KKT_LDL, QpsInfo


class LinearSolverMode(enum.IntEnum):
    """SolveQuadraticProgram.jl:11 (the reference's spelling ``modeItertaive`` is kept)."""
    modeAuto = 1
    modeItertaive = 2
    modeDirect = 3


class ConvergenceFlag(enum.IntEnum):
    """SolveQuadraticProgram.jl:12"""
    convNumItr = 1
    convAdmm = 2
    convPrimDual = 3

    @classmethod
    def _missing_(cls, value):
        """The two additive flags (below) are values of this type without being members of the reference's enum: iterating it still gives the reference's three."""
        name = _ADDITIVE_FLAGS.get(value)
        if name is None:
            return None
        flag = int.__new__(cls, value)
        flag._name_, flag._value_ = name, value
        return cls._value2member_map_.setdefault(value, flag)


# Additive, returned only by a shared-matrix batch with set_infeasibility on (qps_set_shared_infeasibility): QPS_CONV_PRIMAL_INFEASIBLE, QPS_CONV_DUAL_INFEASIBLE.
# ConvergenceFlag(4) is ConvergenceFlag.convPrimInfeasible, an int equal to 4 whose name is "convPrimInfeasible"; likewise 5.
_ADDITIVE_FLAGS = {4: "convPrimInfeasible", 5: "convDualInfeasible"}
ConvergenceFlag.convPrimInfeasible = ConvergenceFlag(4)
ConvergenceFlag.convDualInfeasible = ConvergenceFlag(5)


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


def _vec(v, name, length=None):
    a = np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(-1))
    if length is not None and a.shape[0] != length:
        raise ValueError(f"dimension mismatch: {name} has {a.shape[0]} elements, expected {length}")
    return a


def _validate_dims(numElementsX, mP, vQ, mA, vL, vU):
    """The reference Julia loop never validates (SolveQuadraticProgram.jl:19-24); the MATLAB original does
    (SolveQuadraticProgram.m:158-184) and this mirrors those checks."""
    if mP.shape[0] != mP.shape[1]:
        raise ValueError("The matrix mP must be square")
    if mP.shape[0] != numElementsX:
        raise ValueError("The matrix mP dimensions must match the vector vX")
    if np.asarray(vQ).reshape(-1).shape[0] != numElementsX:
        raise ValueError("The vector vQ dimensions must match the vector vX")
    if mA.shape[1] != numElementsX:
        raise ValueError("The number of columns of mA must match the vector vX")
    if np.asarray(vL).reshape(-1).shape[0] != mA.shape[0] or np.asarray(vU).reshape(-1).shape[0] != mA.shape[0]:
        raise ValueError("The vectors vL, vU dimensions must match the rows of mA")


class _Handle:
    """What every wrapper of a qps_handle shares: profiling, destruction, context-manager use."""
    _h = None

    def set_profiling(self, level: int):
        _lib.check(_lib.lib().qps_set_profiling(self._h, int(level)), self._h)

    def kernel_times(self):
        buf = (_lib.QpsKernelTime * 32)()
        cnt = C.c_int32(0)
        _lib.check(_lib.lib().qps_kernel_times(self._h, buf, 32, C.byref(cnt)), self._h)
        return [dict(name=buf[i].name.decode(), seconds=buf[i].seconds, launches=buf[i].launches, algo_bytes=buf[i].algo_bytes)
                for i in range(cnt.value)]

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().qps_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class QuadraticProgram(_Handle):
    """A problem resident in HBM (qps_create_dense / qps_create_csc ... qps_destroy).

    ``linsys``: "cholesky" (dense reduced form; sparse inputs are densified on the device), "cg" (CSR; CG on the reduced operator: matrix-free
    -- LinOpCg / LinMapsCg -- unless the explicit reduced matrix pays, see include/qps.h), "cg_explicit" (CSR; ItrSolCg: CG on the explicit
    reduced matrix mPI + rho mAA, LinearSystemSolvers.jl:110-142) or "ldl" (CSR, sparse L D L' of the KKT matrix: the reference's direct plugins).
    """

    def __init__(self, mP, vQ, mA, vL, vU, *, linsys="cholesky", dtype="f64", device=0):
        n = mP.shape[0]
        m = mA.shape[0]
        _validate_dims(n, mP, vQ, mA, vL, vU)
        self.n, self.m = n, m
        self.linsys = {"cholesky": QPS_LINSYS_CHOLESKY, "cg": QPS_LINSYS_CG, "cg_explicit": QPS_LINSYS_CG_EXPLICIT, "ldl": QPS_LINSYS_KKT_LDL, "auto": QPS_LINSYS_AUTO}[linsys]
        csr = linsys in ("cg", "cg_explicit", "ldl")
        dt = {"f64": QPS_F64, "f32": QPS_F32}[dtype]
        q, l, u = _vec(vQ, "vQ", n), _vec(vL, "vL", m), _vec(vU, "vU", m)
        h = C.c_void_p()
        L = _lib.lib()
        if sp.issparse(mP) or sp.issparse(mA) or csr:
            Pc = sp.csc_matrix(mP, dtype=np.float64)
            Ac = sp.csc_matrix(mA, dtype=np.float64)
            Pc.sum_duplicates()
            Ac.sum_duplicates()
            Pcp, Pri, Pnz = Pc.indptr.astype(np.int64), Pc.indices.astype(np.int64), np.ascontiguousarray(Pc.data)
            Acp, Ari, Anz = Ac.indptr.astype(np.int64), Ac.indices.astype(np.int64), np.ascontiguousarray(Ac.data)
            st = L.qps_create_csc(n, m, _ip(Pcp), _ip(Pri), _dp(Pnz), _ip(Acp), _ip(Ari), _dp(Anz), _dp(q), _dp(l), _dp(u),
                                  0, 0 if csr else 1, dt, device, C.byref(h))
        else:
            Pd = np.asfortranarray(mP, dtype=np.float64)
            Ad = np.asfortranarray(mA, dtype=np.float64)
            st = L.qps_create_dense(n, m, _dp(Pd), max(n, 1), _dp(Ad), max(m, 1), _dp(q), _dp(l), _dp(u), dt, device, C.byref(h))
        _lib.check(st)
        self._h = h

    # -- SolveQuadraticProgram! -----------------------------------------------------------------------------------
    def solve(self, vX, *, numIterations=5000, ϵAbs=1e-6, ϵRel=1e-6, ρ=1, σ=1e-6, α=1.6, δ=1e-6, adptΡ=False, fctrΡ=5,
              numItrConv=25, numItrPolish=10, ϵMinres=1e-6, numItrMinres=500, ϵPcg=1e-6, numItrPcg=1000,
              trsvBlock=0, reuseFactor=False, loopVariant=0, polish=False, info=None):
        """Mutates ``vX`` (warm start in, solution out) and returns the ConvergenceFlag.  ``polish=True`` appends the
        polishing step of SolveQuadraticProgram.m:289-325 (off by default: the Julia loop reserves its kwargs unused)."""
        if not isinstance(vX, np.ndarray) or vX.dtype != np.float64 or not vX.flags.c_contiguous or vX.shape != (self.n,):
            raise ValueError("vX must be a contiguous float64 vector of length numElements (it is updated in place)")
        p = _lib.default_params()
        p.numIterations, p.epsAbs, p.epsRel = int(numIterations), float(ϵAbs), float(ϵRel)
        p.rho, p.sigma, p.alpha, p.delta = float(ρ), float(σ), float(α), float(δ)
        p.adptRho, p.fctrRho, p.numItrConv = int(bool(adptΡ)), float(fctrΡ), int(numItrConv)
        p.numItrPolish, p.epsMinres, p.numItrMinres = int(numItrPolish), float(ϵMinres), int(numItrMinres)
        p.epsPcg, p.numItrPcg = float(ϵPcg), int(numItrPcg)
        p.linsys, p.trsvBlock, p.reuseFactor = self.linsys, int(trsvBlock), int(bool(reuseFactor))
        p.loopVariant, p.polish = int(loopVariant), int(bool(polish))
        inf = QpsInfo()
        _lib.check(_lib.lib().qps_solve(self._h, _dp(vX), C.byref(p), C.byref(inf)), self._h)
        if info is not None:
            info.update(inf.as_dict())
        return ConvergenceFlag(inf.convFlag)

    def polish(self, vX, vY, *, numItrPolish=10, δ=1e-6, ϵMinres=1e-6, numItrMinres=500):
        """The polishing step alone (SolveQuadraticProgram.m:289-325) from a primal ``vX`` (updated in place when MINRES
        converged) and a multiplier ``vY``.  Returns the report dict (flag 0 = polished, 1 = kept, -1 = did not run)."""
        if not isinstance(vX, np.ndarray) or vX.dtype != np.float64 or not vX.flags.c_contiguous or vX.shape != (self.n,):
            raise ValueError("vX must be a contiguous float64 vector of length numElements (it is updated in place)")
        y = np.ascontiguousarray(vY, dtype=np.float64)
        if y.shape != (self.m,):
            raise ValueError("vY must have length numConstraints")
        p = _lib.default_params()
        p.numItrPolish, p.delta, p.epsMinres, p.numItrMinres, p.polish = int(numItrPolish), float(δ), float(ϵMinres), int(numItrMinres), 1
        rep = _lib.QpsPolishReport()
        _lib.check(_lib.lib().qps_polish(self._h, _dp(vX), _dp(y if self.m else np.zeros(1)), C.byref(p), C.byref(rep)), self._h)
        return rep.as_dict()

    def dual(self):
        """(z, y) of the last solve (additive: the reference discards them)."""
        z = np.zeros(max(self.m, 1))
        y = np.zeros(max(self.m, 1))
        _lib.check(_lib.lib().qps_get_dual(self._h, _dp(z), _dp(y)), self._h)
        return z[:self.m], y[:self.m]

    # -- the literal plugin pair ------------------------------------------------------------------------------------
    def linsys_init(self, ρ, σ, trsvBlock=0):
        _lib.check(_lib.lib().qps_linsys_init(self._h, float(ρ), float(σ), self.linsys, int(trsvBlock)), self._h)

    def linsys_solve(self, vX, vZ, vY, ρ, σ, changedΡ, vXX, vZZ, ϵPcg=None, numItrPcg=None):
        if ϵPcg is not None or numItrPcg is not None:                       # LinOpCg!(...; ϵPcg = 1e-6, numItrPcg = 1000), LinearSystemSolvers.jl:164
            _lib.check(_lib.lib().qps_linsys_set_cg(self._h, float(1e-6 if ϵPcg is None else ϵPcg), int(1000 if numItrPcg is None else numItrPcg)), self._h)
        x, z, y = _vec(vX, "vX", self.n), _vec(vZ, "vZ", self.m), _vec(vY, "vY", self.m)
        xx = np.zeros(self.n)
        zz = np.zeros(max(self.m, 1))
        _lib.check(_lib.lib().qps_linsys_solve(self._h, _dp(x), _dp(z), _dp(y), float(ρ), float(σ), int(bool(changedΡ)),
                                               _dp(xx), _dp(zz)), self._h)
        vXX[:] = xx
        vZZ[:] = zz[:self.m]

    # -- one application of the operator's matrices (qps_operator_apply) ----------------------------------------------
    def apply(self, op, v, ρ=1.0, σ=0.0):
        """``op`` in "P", "A", "At", "PA", "reduced": mP v, mA v, mA' v, [mP; mA] v, (mP + ρ mA'mA + σ I) v (LinearSystemSolvers.jl:152-157) through the
        device kernels this handle's solves use for those products."""
        kind = {"P": _lib.QPS_OP_P, "A": _lib.QPS_OP_A, "At": _lib.QPS_OP_AT, "PA": _lib.QPS_OP_PA, "reduced": _lib.QPS_OP_REDUCED}[op]
        vin = _vec(v, "v", self.m if op == "At" else self.n)
        out = np.zeros(max({"P": self.n, "A": self.m, "At": self.n, "PA": self.n + self.m, "reduced": self.n}[op], 1))
        _lib.check(_lib.lib().qps_operator_apply(self._h, kind, _dp(vin if vin.size else np.zeros(1)), _dp(out), float(ρ), float(σ)), self._h)
        return out[:{"P": self.n, "A": self.m, "At": self.n, "PA": self.n + self.m, "reduced": self.n}[op]]

    # -- profiling ----------------------------------------------------------------------------------------------------

class QuadraticProgramBatch(_Handle):
    """A batch of independent dense QPs of one shape resident in HBM (qps_create_dense_batch / qps_solve_batch):
    the per-problem loop of RunBenchmarks.jl:88-104 advanced in lock step by batched launches.  Every QP keeps its own
    rho, proposed rho, convergence flag and stopping iteration, exactly as if solved alone."""

    def __init__(self, problems, *, dtype="f64", device=0, devices=None, chunk=0):
        """``problems``: sequence of (mP, vQ, mA, vL, vU) tuples with identical shapes (dense or scipy sparse).

        ``devices`` (a list of device ordinals, one entry per worker; a device may appear more than once) selects the in-process multi-device driver
        (qps_solve_batch_multi): one host thread per entry, each taking ranges of at most ``chunk`` QPs from a shared counter (``chunk`` <= 0: one contiguous slab
        per worker).  The problem data then stays on the host and every ``solve`` builds and drops the per-range batch handles; ``dual`` is not available."""
        self.count = len(problems)
        self.devices = None if devices is None else [int(d) for d in devices]
        self.chunk = int(chunk)
        self.worker_of, self.worker_seconds = None, None
        mP0, _, mA0, _, _ = problems[0]
        self.n, self.m = mP0.shape[0], mA0.shape[0]
        dense = lambda M: np.asarray(M.toarray() if sp.issparse(M) else M, dtype=np.float64)
        for (mP, vQ, mA, vL, vU) in problems:
            _validate_dims(self.n, mP, vQ, mA, vL, vU)
            if mA.shape[0] != self.m:
                raise ValueError("all problems of a batch must have the same number of constraints")
        P = np.ascontiguousarray(np.stack([dense(p[0]).ravel(order="F") for p in problems]))
        A = np.ascontiguousarray(np.stack([dense(p[2]).ravel(order="F") for p in problems])) if self.m > 0 else np.zeros((self.count, 1))
        q = np.ascontiguousarray(np.stack([_vec(p[1], "vQ", self.n) for p in problems]))
        l = np.ascontiguousarray(np.stack([_vec(p[3], "vL", self.m) for p in problems])) if self.m > 0 else np.zeros((self.count, 1))
        u = np.ascontiguousarray(np.stack([_vec(p[4], "vU", self.m) for p in problems])) if self.m > 0 else np.zeros((self.count, 1))
        h = C.c_void_p()
        dt = {"f64": QPS_F64, "f32": QPS_F32}[dtype]
        if self.devices is not None:
            if not self.devices:
                raise ValueError("devices must list at least one worker")
            self._host = (P, A, q, l, u, dt)
            self._h = None
            return
        _lib.check(_lib.lib().qps_create_dense_batch(self.count, self.n, self.m, _dp(P), _dp(A), _dp(q), _dp(l), _dp(u), dt, device, C.byref(h)))
        self._h = h

    def _extra_params(self, p):
        """What a subclass adds to the qps_params of ``solve`` (nothing here)."""

    def solve(self, mX=None, *, numIterations=5000, ϵAbs=1e-6, ϵRel=1e-6, ρ=1, σ=1e-6, α=1.6, adptΡ=False, fctrΡ=5, numItrConv=25,
              trsvBlock=0, reuseFactor=False, polish=False, numItrPolish=10, δ=1e-6, ϵMinres=1e-6, numItrMinres=500):
        """Returns (mX [count x n], list of ConvergenceFlag, list of info dicts).  ``mX`` (optional) holds the warm starts."""
        X = np.zeros((self.count, self.n)) if mX is None else np.ascontiguousarray(mX, dtype=np.float64).copy()
        p = _lib.default_params()
        p.numIterations, p.epsAbs, p.epsRel = int(numIterations), float(ϵAbs), float(ϵRel)
        p.rho, p.sigma, p.alpha = float(ρ), float(σ), float(α)
        p.adptRho, p.fctrRho, p.numItrConv = int(bool(adptΡ)), float(fctrΡ), int(numItrConv)
        p.trsvBlock, p.reuseFactor = int(trsvBlock), int(bool(reuseFactor))
        p.polish, p.numItrPolish, p.delta, p.epsMinres, p.numItrMinres = int(bool(polish)), int(numItrPolish), float(δ), float(ϵMinres), int(numItrMinres)
        infos = (QpsInfo * self.count)()
        if self.devices is not None:
            P, A, q, l, u, dt = self._host
            W = len(self.devices)
            devs = (C.c_int32 * W)(*self.devices)
            owner = (C.c_int32 * self.count)()
            secs = (C.c_double * W)()
            _lib.check(_lib.lib().qps_solve_batch_multi(self.count, self.n, self.m, _dp(P), _dp(A), _dp(q), _dp(l), _dp(u), dt, devs, W, self.chunk, _dp(X), C.byref(p), infos,
                                                        owner, secs))
            self.worker_of, self.worker_seconds = list(owner), list(secs)
            return X, [ConvergenceFlag(i.convFlag) for i in infos], [i.as_dict() for i in infos]
        _lib.check(_lib.lib().qps_solve_batch(self._h, _dp(X), C.byref(p), infos), self._h)
        return X, [ConvergenceFlag(i.convFlag) for i in infos], [i.as_dict() for i in infos]

    def dual(self):
        """(mZ, mY) [count x m] of the last solve (additive: the reference discards them)."""
        if self.devices is not None:
            raise RuntimeError("dual() is not available in multi-device mode (the per-range handles are dropped after their solve)")
        Z = np.zeros((self.count, max(self.m, 1)))
        Y = np.zeros((self.count, max(self.m, 1)))
        if self.m > 0:
            _lib.check(_lib.lib().qps_get_dual(self._h, _dp(Z), _dp(Y)), self._h)
        return Z[:, :self.m], Y[:, :self.m]


def equality_rho_scale(mL, mU, factor=1e3):
    """The ρ scale of OSQP §5.2 for a family: ``factor`` on the rows that are equalities (l == u) in EVERY column of ``mL`` / ``mU`` ([count x m], or one
    vector of length m), 1 elsewhere.  What ``QuadraticProgramSharedBatch.set_rho_scale`` takes."""
    L, U = np.atleast_2d(np.asarray(mL, dtype=np.float64)), np.atleast_2d(np.asarray(mU, dtype=np.float64))
    if L.shape != U.shape:
        raise ValueError(f"dimension mismatch: mL has shape {L.shape}, mU has shape {U.shape}")
    return np.where(np.all(L == U, axis=0), float(factor), 1.0)


class QuadraticProgramSharedBatch(_Handle):
    """``count`` QPs on ONE ``mP`` and ONE ``mA`` that differ in ``q``, ``l`` and ``u`` only (qps_create_dense_shared_batch): an MPC horizon
    re-solved every sample, a regularisation path, a scenario sweep.  ``mQ`` is [count x n], ``mL`` / ``mU`` are [count x m].  The matrices are
    stored, factorised and streamed once for all columns; every column keeps its own check, flag, stopping iteration and residuals, exactly as if
    solved alone with a fixed ρ (``adptΡ``, ``polish`` and a ``trsvBlock`` below n are refused with QPS_ERR_UNSUPPORTED); ``set_adaptive_rho`` lets one ρ adapt
    for the whole family."""

    def __init__(self, mP, mA, mQ, mL, mU, *, dtype="f64", device=0):
        dense = lambda M: np.asarray(M.toarray() if sp.issparse(M) else M, dtype=np.float64)
        mP, mA = dense(mP), dense(mA)
        if mP.ndim != 2 or mA.ndim != 2:
            raise ValueError("mP and mA must be matrices")
        self.n, self.m = mP.shape[0], mA.shape[0]
        q = np.ascontiguousarray(np.atleast_2d(np.asarray(mQ, dtype=np.float64)))
        self.count = q.shape[0]
        l, u = self._rows(mL, "mL", self.m), self._rows(mU, "mU", self.m)
        for b in range(self.count):
            _validate_dims(self.n, mP, q[b], mA, l[b], u[b])
        Pd, Ad = np.asfortranarray(mP), np.asfortranarray(mA)
        h = C.c_void_p()
        dt = {"f64": QPS_F64, "f32": QPS_F32}[dtype]
        _lib.check(_lib.lib().qps_create_dense_shared_batch(self.count, self.n, self.m, _dp(Pd), max(self.n, 1), _dp(Ad), max(self.m, 1),
                                                            _dp(q), _dp(l), _dp(u), dt, device, C.byref(h)))
        self._h = h

    _linsys = QPS_LINSYS_AUTO          # what solve() passes as qps_params.linsys (the library's default)

    def _rows(self, M, name, length):
        a = np.ascontiguousarray(np.atleast_2d(np.asarray(M, dtype=np.float64)))
        if a.shape != (self.count, length):
            raise ValueError(f"dimension mismatch: {name} has shape {a.shape}, expected {(self.count, length)}")
        return a

    def update(self, mQ=None, mL=None, mU=None):
        """Replaces q, l and / or u of every column (``None`` keeps the array).  The factorisation does not depend on them: a following
        ``solve(reuseFactor=True)`` with unchanged (ρ, σ) does not factorise again."""
        q = None if mQ is None else self._rows(mQ, "mQ", self.n)
        l = None if mL is None else self._rows(mL, "mL", self.m)
        u = None if mU is None else self._rows(mU, "mU", self.m)
        ptr = lambda a: None if a is None else _dp(a)
        _lib.check(_lib.lib().qps_update_shared_vectors(self._h, ptr(q), ptr(l), ptr(u)), self._h)

    def update_matrices(self, mP=None, mA=None):
        """Replaces the values of ``mP`` and / or ``mA`` in place (qps_update_shared_matrices; ``None`` keeps that matrix): same shapes as at creation.  Every option,
        q, l, u, the stored z and y and all allocations stay, so ``set_warm_start("state")`` carries on across the change; the next ``solve`` factorises, also with
        ``reuseFactor=True`` (with it, an update of ``mP`` alone skips the product A'A).  With equilibration on, the handle keeps its D and E; ``set_equilibration``
        again computes them from the new matrices.  A refused call leaves the handle as it was."""
        dense = lambda M: np.asfortranarray(np.asarray(M.toarray() if sp.issparse(M) else M, dtype=np.float64))
        Pd = None if mP is None else dense(mP)
        Ad = None if mA is None else dense(mA)
        if Pd is not None and Pd.shape != (self.n, self.n):
            raise ValueError(f"dimension mismatch: mP has shape {Pd.shape}, expected {(self.n, self.n)}")
        if Ad is not None and Ad.shape != (self.m, self.n):
            raise ValueError(f"dimension mismatch: mA has shape {Ad.shape}, expected {(self.m, self.n)}")
        ptr = lambda a: None if a is None else _dp(a)
        _lib.check(_lib.lib().qps_update_shared_matrices(self._h, ptr(Pd), max(self.n, 1), ptr(Ad), max(self.m, 1)), self._h)

    def set_rho_scale(self, vS=None):
        """Per-constraint ρ scale shared by all columns (qps_set_shared_rho_scale): row i runs with ρ_i = ρ vS[i]; ``vS`` has m finite, strictly
        positive entries (``equality_rho_scale`` builds the usual one).  ``None`` goes back to the scalar ρ.  Either way the next ``solve``
        factorises, also with ``reuseFactor=True``; ``ρ`` of ``solve`` stays the base value."""
        s = None if vS is None else _vec(vS, "vS", self.m)
        _lib.check(_lib.lib().qps_set_shared_rho_scale(self._h, None if s is None else _dp(s)), self._h)

    def set_adaptive_rho(self, on=True):
        """Family-wide adaptive ρ (qps_set_shared_adaptive_rho): ONE ρ that moves for all columns by the reference's rule, with the norms of the worst
        columns still running; a switch re-factorises once for the whole batch and uses ``fctrΡ`` of ``solve``.  ``False`` goes back to the fixed ρ.
        The setting stays with the handle.  Per column, ``numRefactor`` / ``rhoFinal`` / ``rhoProposed`` / ``tRefactor`` of the info dicts report it;
        ``solve(reuseFactor=True, ρ=rhoFinal)`` of the column that ran longest re-solves without factorising.  ``adptΡ=True`` (the per-problem rule)
        stays refused."""
        _lib.check(_lib.lib().qps_set_shared_adaptive_rho(self._h, 1 if on else 0), self._h)

    def set_column_rho(self, on=True):
        """Per-column adaptive ρ (qps_set_shared_column_rho), on ``QuadraticProgramCgSharedBatch``: every column moves its OWN ρ by the reference's rule
        (SolveQuadraticProgram.jl:47, :92-96) from its own four norms, starting from ``ρ`` of every ``solve`` and switching on ``fctrΡ``; nothing is factorised
        there, so a switch is one small upload.  A column then equals ``QuadraticProgram(..., linsys="cg", adptΡ=True)``; ``numRefactor`` / ``rhoFinal`` /
        ``rhoProposed`` of the info dicts are the column's own.  The batch still runs until its slowest column.  ``False`` goes back to the fixed ρ.  The setting
        stays with the handle and excludes ``set_adaptive_rho`` (turn the other off first).  The dense and the sparse L D L' handle refuse it with
        QPS_ERR_UNSUPPORTED: one factor serves every column there."""
        _lib.check(_lib.lib().qps_set_shared_column_rho(self._h, 1 if on else 0), self._h)

    def set_equilibration(self, passes=10):
        """Ruiz equilibration with exact powers of two (qps_set_shared_equilibration; OSQP §5.1), opt-in: ``passes`` = 1..50 passes of the rule, computed once for the
        family from mP and mA; ``0`` or ``None`` switches it off and restores the matrices bit for bit.  The loop runs on D P D, E A D, D q, E l, E u; warm starts,
        results, ``dual()`` and the convergence check stay in the caller's units.  Setting, changing or clearing makes the next ``solve`` factorise, also with
        ``reuseFactor=True``.  QPS_ERR_UNSUPPORTED when a scaled matrix entry would leave the normal range of the handle's type (the handle stays as it was)."""
        _lib.check(_lib.lib().qps_set_shared_equilibration(self._h, 0 if passes is None else int(passes)), self._h)

    def equilibration(self):
        """(vD [n], vE [m]) of ``set_equilibration``: powers of two, all ones while it is off (qps_get_shared_equilibration)."""
        vD, vE = np.zeros(self.n), np.zeros(self.m)
        _lib.check(_lib.lib().qps_get_shared_equilibration(self._h, _dp(vD), _dp(vE)), self._h)
        return vD, vE

    _WARM_MODES = {None: 0, False: 0, "off": 0, True: 1, "state": 1, "ax": 2}

    def set_warm_start(self, mode="state"):
        """Warm start of z and y across re-solves (qps_set_shared_warm_start), opt-in.  ``None`` / ``False`` / ``"off"``: every ``solve`` restarts z = y = 0 (the
        default).  ``True`` / ``"state"``: every column starts from the z and y the handle holds -- those of its own stopping iteration of the last ``solve``, or
        what ``set_dual`` wrote since -- and from ``mX``.  ``"ax"``: OSQP's warm_start(x, y); y from the handle, z = A x formed on the device from ``mX``.  The
        setting stays with the handle; with ``update`` and ``solve(reuseFactor=True)`` a re-solve neither factorises nor starts its iterations over."""
        if isinstance(mode, (bool, str, type(None))):
            if mode not in self._WARM_MODES:
                raise ValueError(f"mode must be one of None, False, 'off', True, 'state', 'ax' (got {mode!r})")
            mode = self._WARM_MODES[mode]
        _lib.check(_lib.lib().qps_set_shared_warm_start(self._h, int(mode)), self._h)

    def set_dual(self, mZ=None, mY=None):
        """Writes z and / or y of every column ([count x m], the caller's units; qps_set_shared_dual, the counterpart of ``dual``).  ``None`` keeps that array."""
        z = None if mZ is None else self._rows(mZ, "mZ", self.m)
        y = None if mY is None else self._rows(mY, "mY", self.m)
        ptr = lambda a: None if a is None else _dp(a)
        _lib.check(_lib.lib().qps_set_shared_dual(self._h, ptr(z), ptr(y)), self._h)

    def set_infeasibility(self, ϵPrimInf=1e-4, ϵDualInf=1e-4):
        """Per-column infeasibility certificates (qps_set_shared_infeasibility; OSQP §3.4), opt-in.  At a check, a column that CheckConvergence leaves running is
        tested on the differences of its consecutive iterates: ``convPrimInfeasible`` (4) or ``convDualInfeasible`` (5) stops it there like any other flag, so one
        column without a solution no longer holds the batch to ``numIterations`` nor steers the family-wide ρ.  Each tolerance is finite and >= 0 (OSQP: 1e-4);
        ``None`` / ``False`` / ``0`` leaves that test off, both off is the default and the untouched path.  The setting stays with the handle."""
        eps = [0.0 if (e is None or e is False) else float(e) for e in (ϵPrimInf, ϵDualInf)]
        _lib.check(_lib.lib().qps_set_shared_infeasibility(self._h, eps[0], eps[1]), self._h)

    def certificate(self):
        """(mDY [count x m], mDX [count x n]) of the last ``solve`` (qps_get_shared_certificate): row b of mDY is the projected δy of column b if it ended with
        ``convPrimInfeasible``, row b of mDX its δx if it ended with ``convDualInfeasible``, zeros otherwise; the caller's units, unnormalised."""
        DY, DX = np.zeros((self.count, self.m)), np.zeros((self.count, self.n))
        _lib.check(_lib.lib().qps_get_shared_certificate(self._h, _dp(DY), _dp(DX)), self._h)
        return DY, DX

    def polish(self, mX, mY=None, *, numItrPolish=10, δ=1e-6, ϵMinres=1e-6, numItrMinres=500):
        """The polishing step (SolveQuadraticProgram.m:289-325) for every column at once (qps_polish_shared), from the primals ``mX`` [count x n] (row b is replaced
        in place only where its report has flag 0) and the multipliers ``mY`` [count x m]; ``None`` takes the y the handle holds (the last ``solve`` or
        ``set_dual``).  Returns the list of report dicts, keys as ``QuadraticProgram.polish`` (``seconds``: wall time of the whole batch's step).  Nothing the handle
        keeps is touched; with equilibration on, ``δ`` and ``ϵMinres`` act in the scaled variables."""
        if not isinstance(mX, np.ndarray) or mX.dtype != np.float64 or not mX.flags.c_contiguous or mX.shape != (self.count, self.n):
            raise ValueError("mX must be a contiguous float64 array of shape (count, numElements) (it is updated in place)")
        y = None if mY is None else self._rows(mY, "mY", self.m)
        p = _lib.default_params()
        p.numItrPolish, p.delta, p.epsMinres, p.numItrMinres = int(numItrPolish), float(δ), float(ϵMinres), int(numItrMinres)
        reps = (_lib.QpsPolishReport * self.count)()
        _lib.check(_lib.lib().qps_polish_shared(self._h, _dp(mX), None if y is None else _dp(y), C.byref(p), reps), self._h)
        return [r.as_dict() for r in reps]

    _value_gradients = False   # the classes created from CSC arrays keep a pattern and give vP / vA

    def adjoint(self, mGX, mX, mY=None, *, numItrPolish=10, δ=1e-6, ϵMinres=1e-6, numItrMinres=500, matrices=True):
        """Adjoint derivatives of the solution for every column at once (qps_adjoint_shared; OSQP's ``adjoint_derivative_compute``): from ``mGX`` [count x n], the
        gradient of a loss with respect to each column's solution, the solutions ``mX`` [count x n] and the multipliers ``mY`` [count x m] (``None`` takes the y
        the handle holds), the gradient of that loss with respect to the data.  Per column the reduced KKT system of the polishing step on the active rows of y is
        solved for the right-hand side [g_x; 0] by its refinement rounds.  Returns ``dict(dQ, dL, dU, vP, vA, reports)``: ``dQ`` [count x n], ``dL`` / ``dU``
        [count x m] per column; ``vP`` / ``vA`` the gradients with respect to the stored values of ``mP`` (over symmetric perturbations) and ``mA``, summed over
        the columns, in the order of ``pattern()`` and ``update_values`` -- ``None`` on the dense handle or with ``matrices=False``; ``reports`` as ``polish``.  A
        column whose report has a flag other than 0 has zero rows and is left out of ``vP`` / ``vA``.  Nothing the handle keeps is touched; with equilibration
        on, ``δ`` and ``ϵMinres`` act in the scaled variables and every result is in the caller's units."""
        gx, x = self._rows(mGX, "mGX", self.n), self._rows(mX, "mX", self.n)
        y = None if mY is None else self._rows(mY, "mY", self.m)
        p = _lib.default_params()
        p.numItrPolish, p.delta, p.epsMinres, p.numItrMinres = int(numItrPolish), float(δ), float(ϵMinres), int(numItrMinres)
        dQ, dL, dU = np.zeros((self.count, self.n)), np.zeros((self.count, self.m)), np.zeros((self.count, self.m))
        vP = vA = None
        if matrices and self._value_gradients:
            nP, nA = C.c_int64(), C.c_int64()
            _lib.check(_lib.lib().qps_get_shared_pattern(self._h, C.byref(nP), C.byref(nA), None, None, None, None), self._h)
            vP, vA = np.zeros(nP.value), np.zeros(nA.value)
        reps = (_lib.QpsPolishReport * self.count)()
        ptr = lambda a: None if a is None else _dp(a)
        _lib.check(_lib.lib().qps_adjoint_shared(self._h, _dp(x), ptr(y), _dp(gx), C.byref(p), _dp(dQ), _dp(dL), _dp(dU), ptr(vP), ptr(vA), reps), self._h)
        return dict(dQ=dQ, dL=dL, dU=dU, vP=vP, vA=vA, reports=[r.as_dict() for r in reps])

    def set_polish(self, on=True):
        """``True``: every ``solve`` ends with the polishing step on its own x and y (qps_set_shared_polish), with ``numItrPolish``, ``δ``, ``ϵMinres`` and
        ``numItrMinres`` of that ``solve``; ``polishFlag`` / ``polishIterations`` / ``tPolish`` of the info dicts report it per column, and a column that ended with
        an infeasibility flag is left alone.  ``False`` (the default): as without it.  ``polish=True`` of ``solve`` stays refused."""
        _lib.check(_lib.lib().qps_set_shared_polish(self._h, 1 if on else 0), self._h)

    def _extra_params(self, p):
        """What a subclass adds to the qps_params of ``solve`` (nothing here)."""

    def solve(self, mX=None, *, numIterations=5000, ϵAbs=1e-6, ϵRel=1e-6, ρ=1, σ=1e-6, α=1.6, adptΡ=False, fctrΡ=5, numItrConv=25,
              trsvBlock=0, reuseFactor=False, polish=False, numItrPolish=10, δ=1e-6, ϵMinres=1e-6, numItrMinres=500):
        """Returns (mX [count x n], list of ConvergenceFlag, list of info dicts), as ``QuadraticProgramBatch.solve``.  ``mX`` (optional) holds the warm starts."""
        X = np.zeros((self.count, self.n)) if mX is None else np.ascontiguousarray(mX, dtype=np.float64).copy()
        if X.shape != (self.count, self.n):
            raise ValueError(f"dimension mismatch: mX has shape {X.shape}, expected {(self.count, self.n)}")
        p = _lib.default_params()
        p.numIterations, p.epsAbs, p.epsRel = int(numIterations), float(ϵAbs), float(ϵRel)
        p.rho, p.sigma, p.alpha = float(ρ), float(σ), float(α)
        p.adptRho, p.fctrRho, p.numItrConv = int(bool(adptΡ)), float(fctrΡ), int(numItrConv)
        p.trsvBlock, p.reuseFactor = int(trsvBlock), int(bool(reuseFactor))
        p.polish, p.numItrPolish, p.delta, p.epsMinres, p.numItrMinres = int(bool(polish)), int(numItrPolish), float(δ), float(ϵMinres), int(numItrMinres)
        p.linsys = self._linsys
        self._extra_params(p)
        infos = (QpsInfo * self.count)()
        _lib.check(_lib.lib().qps_solve_batch(self._h, _dp(X), C.byref(p), infos), self._h)
        return X, [ConvergenceFlag(i.convFlag) for i in infos], [i.as_dict() for i in infos]

    def dual(self):
        """(mZ, mY) [count x m] of the last solve (additive: the reference discards them)."""
        Z = np.zeros((self.count, self.m))
        Y = np.zeros((self.count, self.m))
        _lib.check(_lib.lib().qps_get_dual(self._h, _dp(Z), _dp(Y)), self._h)
        return Z, Y


class QuadraticProgramSparseSharedBatch(QuadraticProgramSharedBatch):
    """``count`` QPs on ONE sparse ``mP`` and ONE sparse ``mA`` (qps_create_csc_shared_batch): the lasso / Huber / SVM regularisation paths and scenario
    sweeps whose matrices are too large and too sparse for the reduced dense form.  ``mP`` / ``mA`` are scipy sparse or dense and go to the library as
    CSC; ``mQ`` is [count x n], ``mL`` / ``mU`` are [count x m].  The linear system is the sparse L D L' of the KKT matrix: ordering and symbolic factor
    once at creation, one numeric factorisation for all columns, every iteration sweeps 16 columns per launch.  Every column behaves as a stand-alone
    ``QuadraticProgram(..., linsys="ldl")`` solve with a fixed ρ (``adptΡ``, ``polish`` and a ``linsys`` other than "auto" / "ldl" are refused with
    QPS_ERR_UNSUPPORTED; ``trsvBlock`` is accepted and without effect).  ``update``, ``solve`` and ``dual`` are those of ``QuadraticProgramSharedBatch``."""

    _create = "qps_create_csc_shared_batch"    # the entry point that takes the CSC arrays
    _value_gradients = True

    def __init__(self, mP, mA, mQ, mL, mU, *, dtype="f64", device=0):
        if getattr(mP, "ndim", 0) != 2 or getattr(mA, "ndim", 0) != 2:
            raise ValueError("mP and mA must be matrices")
        self.n, self.m = mP.shape[0], mA.shape[0]
        self._device = int(device)                                 # update_values holds device tensors against it
        q = np.ascontiguousarray(np.atleast_2d(np.asarray(mQ, dtype=np.float64)))
        self.count = q.shape[0]
        l, u = self._rows(mL, "mL", self.m), self._rows(mU, "mU", self.m)
        _validate_dims(self.n, mP, q[0], mA, l[0], u[0])          # (every row of mQ / mL / mU has the length of the first)
        (Pcp, Pri, Pnz), (Acp, Ari, Anz) = self._csc(mP), self._csc(mA)
        h = C.c_void_p()
        dt = {"f64": QPS_F64, "f32": QPS_F32}[dtype]
        _lib.check(getattr(_lib.lib(), self._create)(self.count, self.n, self.m, _ip(Pcp), _ip(Pri), _dp(Pnz), _ip(Acp), _ip(Ari), _dp(Anz),
                                                      _dp(q), _dp(l), _dp(u), 0, dt, device, C.byref(h)))
        self._h = h

    @staticmethod
    def _csc(M):
        """(colptr, rowval, nzval) as the library takes them: what ``scipy.sparse.csc_matrix`` makes of ``M``, duplicates summed -- the same input gives the same
        stored pattern at creation and at ``update_matrices`` (an explicit zero stays an entry)."""
        Mc = sp.csc_matrix(M, dtype=np.float64)
        Mc.sum_duplicates()
        return Mc.indptr.astype(np.int64), Mc.indices.astype(np.int64), np.ascontiguousarray(Mc.data)

    def update_matrices(self, mP=None, mA=None):
        """Replaces the values of ``mP`` and / or ``mA`` in place (qps_update_shared_matrices_csc; ``None`` keeps that matrix): anything ``scipy.sparse.csc_matrix``
        accepts, with the shape and the stored pattern of creation (QPS_ERR_BAD_ARGUMENT names the matrix and the first column that differs).  Ordering, symbolic
        factor, every option, q, l, u and the stored z and y stay; the next ``solve`` runs the numeric factorisation, also with ``reuseFactor=True``.  With
        equilibration on, the handle keeps its D and E.  A refused call leaves the handle as it was."""
        for M, name, shape in ((mP, "mP", (self.n, self.n)), (mA, "mA", (self.m, self.n))):
            if M is not None and tuple(getattr(M, "shape", ())) != shape:
                raise ValueError(f"dimension mismatch: {name} has shape {getattr(M, 'shape', None)}, expected {shape}")
        Pcp, Pri, Pnz = (None, None, None) if mP is None else self._csc(mP)
        Acp, Ari, Anz = (None, None, None) if mA is None else self._csc(mA)
        ip, dp = (lambda a: None if a is None else _ip(a)), (lambda a: None if a is None else _dp(a))
        _lib.check(_lib.lib().qps_update_shared_matrices_csc(self._h, ip(Pcp), ip(Pri), dp(Pnz), ip(Acp), ip(Ari), dp(Anz), 0), self._h)

    def pattern(self):
        """``(P_indptr, P_indices, A_indptr, A_indices)`` as int64 arrays (qps_get_shared_pattern): the canonical CSC pattern the handle was created on -- 0-based,
        rows sorted inside every column, duplicates summed, explicit zeros kept.  It never changes; ``update_values`` takes its values in this order."""
        L = _lib.lib()
        nP, nA = C.c_int64(), C.c_int64()
        _lib.check(L.qps_get_shared_pattern(self._h, C.byref(nP), C.byref(nA), None, None, None, None), self._h)
        Pcp, Pri = np.zeros(self.n + 1, dtype=np.int64), np.zeros(nP.value, dtype=np.int64)
        Acp, Ari = np.zeros(self.n + 1, dtype=np.int64), np.zeros(nA.value, dtype=np.int64)
        _lib.check(L.qps_get_shared_pattern(self._h, None, None, _ip(Pcp), _ip(Pri), _ip(Acp), _ip(Ari)), self._h)
        return Pcp, Pri, Acp, Ari

    def update_values(self, vP=None, vA=None):
        """New values of ``mP`` and / or ``mA`` on the stored pattern, in the order of ``pattern()`` (qps_update_shared_values; ``None`` keeps that matrix): the
        host passes of ``update_matrices`` over a pattern that cannot have changed are skipped, and what has to hold for values -- finite, ``mP`` symmetric with
        tolerance 0, the range under kept exponents -- is tested on the device before the handle is touched, with the codes and messages of
        ``update_matrices``.  Each of ``vP``, ``vA`` is anything ``np.asarray(..., float64)`` makes a vector of, or a ``torch.Tensor`` that is float64,
        contiguous and on the handle's device, whose memory the library reads in place (torch's current stream on that device is synchronised first); both
        given, they are both host arrays or both tensors.  The result equals ``update_matrices`` on the same values bit for bit."""
        tensors = [type(v).__module__.split(".")[0] == "torch" for v in (vP, vA) if v is not None]
        if any(tensors) and not all(tensors):
            raise ValueError("vP and vA must both be host arrays or both be torch tensors")
        device = bool(tensors) and tensors[0]
        if device:
            import torch                                                   # only here: host input never needs it
            dev = self._device
            for v, name in ((vP, "vP"), (vA, "vA")):
                if v is None:
                    continue
                if v.dtype != torch.float64:
                    raise ValueError(f"{name} must be a float64 tensor, not {v.dtype}")
                if v.device.type != "cuda" or v.device.index != dev:
                    raise ValueError(f"{name} must be on the handle's device cuda:{dev}, not {v.device}")
                if v.dim() != 1 or not v.is_contiguous():
                    raise ValueError(f"{name} must be a contiguous vector")
            torch.cuda.current_stream(dev).synchronize()                   # the contract of QPS_MEM_DEVICE: the producing work has completed
            args = [(None, 0) if v is None else (v.data_ptr(), v.numel()) for v in (vP, vA)]
        else:
            keep = tuple(None if v is None else np.ascontiguousarray(np.asarray(v, dtype=np.float64)) for v in (vP, vA))
            for v, name in zip(keep, ("vP", "vA")):
                if v is not None and v.ndim != 1:
                    raise ValueError(f"{name} must be a vector")
            args = [(None, 0) if v is None else (v.ctypes.data, v.size) for v in keep]   # keep: alive until the call returns
        (pP, kP), (pA, kA) = args
        _lib.check(_lib.lib().qps_update_shared_values(self._h, pP, kP, pA, kA, _lib.QPS_MEM_DEVICE if device else _lib.QPS_MEM_HOST), self._h)

    def solve(self, mX=None, *, linsys="auto", **kw):
        """As ``QuadraticProgramSharedBatch.solve``; ``linsys`` ("auto" or "ldl": the sparse L D L' either way) goes to the library as it is."""
        self._linsys = {"cholesky": QPS_LINSYS_CHOLESKY, "cg": QPS_LINSYS_CG, "cg_explicit": QPS_LINSYS_CG_EXPLICIT, "ldl": QPS_LINSYS_KKT_LDL, "auto": QPS_LINSYS_AUTO}[linsys]
        return super().solve(mX, **kw)


class QuadraticProgramCgSharedBatch(QuadraticProgramSparseSharedBatch):
    """``count`` QPs on ONE sparse ``mP`` and ONE sparse ``mA`` with the matrix-free CG plugin as their linear system (qps_create_csc_shared_batch_cg): for
    patterns that fill in under any ordering, which ``QuadraticProgramSparseSharedBatch`` refuses or cannot afford.  Constructor and arrays are those of
    ``QuadraticProgramSparseSharedBatch``.  Nothing is factorised: every iteration runs one CG per column, all columns in lockstep, the matrices read once per CG
    iteration for 16 columns.  Every column behaves as a stand-alone ``QuadraticProgram(..., linsys="cg")`` solve (matrix-free) with a fixed ρ and reports its
    own ``cgIterations``; ``adptΡ``, ``polish`` and a ``linsys`` other than "auto" / "cg" are refused with QPS_ERR_UNSUPPORTED, ``set_equilibration`` with a
    positive pass count too.  Every other option of ``QuadraticProgramSharedBatch`` works as there; a ρ switch of ``set_adaptive_rho`` costs no factorisation, and
    ``set_column_rho`` gives every column the reference's per-problem adaptive ρ (a column then equals ``linsys="cg", adptΡ=True``)."""

    _create = "qps_create_csc_shared_batch_cg"
    _cg = (1e-6, 1000)

    def _extra_params(self, p):
        p.epsPcg, p.numItrPcg = float(self._cg[0]), int(self._cg[1])

    def solve(self, mX=None, *, linsys="auto", ϵPcg=1e-6, numItrPcg=1000, **kw):
        """As ``QuadraticProgramSharedBatch.solve``; ``ϵPcg`` and ``numItrPcg`` are abstol and maxiter of every column's CG (LinearSystemSolvers.jl:164),
        ``linsys`` is "auto" or "cg"."""
        self._cg = (ϵPcg, numItrPcg)
        return super().solve(mX, linsys=linsys, **kw)


# ------------------------------------------------------------------------------------------------------------------
# Plugin pairs with the reference signature (LinearSystemSolvers.jl:16,28)
# ------------------------------------------------------------------------------------------------------------------
def _make_pair(linsys: str, dtype: str = "f64"):
    def Init(vX, mP, vQ, mA, ρ, ρ1, σ, numElements, numConstraints):
        # vL/vU are not part of the plugin signature and the linear solve does not need them
        prob = QuadraticProgram(mP, vQ, mA, np.zeros(numConstraints), np.zeros(numConstraints), linsys=linsys, dtype=dtype)
        prob.linsys_init(ρ, σ)
        vXX = np.zeros(numElements)
        vZZ = np.zeros(numConstraints)
        return vXX, vZZ, [prob]

    if linsys in ("cg", "cg_explicit"):
        def Sol(tuSolver, vXX, vZZ, vX, mP, vQ, mA, vZ, vY, ρ, ρ1, σ, numElements, numConstraints, changedΡ, *, ϵPcg=1e-6, numItrPcg=1000):
            tuSolver[0].linsys_solve(vX, vZ, vY, ρ, σ, changedΡ, vXX, vZZ, ϵPcg=ϵPcg, numItrPcg=numItrPcg)    # kwargs of LinearSystemSolvers.jl:164
    else:
        def Sol(tuSolver, vXX, vZZ, vX, mP, vQ, mA, vZ, vY, ρ, ρ1, σ, numElements, numConstraints, changedΡ):
            tuSolver[0].linsys_solve(vX, vZ, vY, ρ, σ, changedΡ, vXX, vZZ)

    Init._qps_linsys = Sol._qps_linsys = linsys
    Init._qps_dtype = Sol._qps_dtype = dtype
    return Init, Sol


HipCholInit, HipChol = _make_pair("cholesky")
HipCgInit, HipCg = _make_pair("cg")
HipItrSolCgInit, HipItrSolCg = _make_pair("cg_explicit")   # ItrSolCgInit / ItrSolCg!: cg! on the explicit reduced matrix (LinearSystemSolvers.jl:110-142)
HipLdlInit, HipLdl = _make_pair("ldl")          # sparse L D L' of the KKT matrix: LaLdl / QDLdl / FacLdl (LinearSystemSolvers.jl:16-107)
HipCholF32Init, HipCholF32 = _make_pair("cholesky", "f32")


def SolveQuadraticProgramInplace(vX, mP, vQ, mA, vL, vU, LinSysSolInit=HipCholInit, LinSysSol=HipChol, *,
                                 numIterations=5000, ϵAbs=1e-6, ϵRel=1e-6, ρ=1, σ=1e-6, α=1.6, δ=1e-6, adptΡ=False,
                                 fctrΡ=5, numItrConv=25, numItrPolish=10, ϵMinres=1e-6, numItrMinres=500, info=None,
                                 device=0, trsvBlock=0, loopVariant=0, polish=False):
    """``SolveQuadraticProgram!`` (SolveQuadraticProgram.jl:14-76): mutates ``vX``, returns the ConvergenceFlag.

    ``δ, numItrPolish, ϵMinres, numItrMinres`` are accepted and, as in the reference (:16-17, no polish), unused unless
    ``polish=True`` asks for the polishing step of the MATLAB implementation (SolveQuadraticProgram.m:289-325).
    ``info`` (optional dict) receives iterations, final ρ, residuals, timings -- additive."""
    linsys = getattr(LinSysSolInit, "_qps_linsys", None)
    if linsys is None or getattr(LinSysSol, "_qps_linsys", None) != linsys:
        raise TypeError("LinSysSolInit/LinSysSol must be one of this package's pairs (HipCholInit, HipChol) / "
                        "(HipCgInit, HipCg) / (HipItrSolCgInit, HipItrSolCg) / (HipLdlInit, HipLdl): the device-resident loop has no CPU path")
    with QuadraticProgram(mP, vQ, mA, vL, vU, linsys=linsys, dtype=LinSysSolInit._qps_dtype, device=device) as prob:
        return prob.solve(vX, numIterations=numIterations, ϵAbs=ϵAbs, ϵRel=ϵRel, ρ=ρ, σ=σ, α=α, δ=δ, adptΡ=adptΡ,
                          fctrΡ=fctrΡ, numItrConv=numItrConv, numItrPolish=numItrPolish, ϵMinres=ϵMinres,
                          numItrMinres=numItrMinres, trsvBlock=trsvBlock, loopVariant=loopVariant, polish=polish, info=info)


SolveQuadraticProgram_b = SolveQuadraticProgramInplace


def AutoLinearSolverMode(mP, mA):
    """The ``modeAuto`` rule of the reference (SolveQuadraticProgram.jl:129-130, :143-151; SolveQuadraticProgram.m:190-199),
    literally: direct when ``numRowsL = rows(P) + rows(A) <= 5000`` and ``(nnz(P) + nnz(A)) / numRowsL^2 <= 0.4``, else iterative.
    Evaluated by the library (``qps_linsys_auto``) so that every binding shares one rule.  ``nnz`` of a dense array counts its
    non-zero entries, as Julia's / MATLAB's ``nnz`` does."""
    nnz = lambda M: int(M.nnz) if sp.issparse(M) else int(np.count_nonzero(M))
    kind = _lib.lib().qps_linsys_auto(mP.shape[0], mA.shape[0], nnz(mP), nnz(mA), int(sp.issparse(mP) and sp.issparse(mA)))
    return LinearSolverMode.modeItertaive if kind == QPS_LINSYS_CG else LinearSolverMode.modeDirect


def SolveQuadraticProgram(mP, vQ, mA, vL, vU, *, linearSolverMode=LinearSolverMode.modeAuto, **kw):
    """Convenience form spelled in BASELINE.json's north_star: ``SolveQuadraticProgram(P, q, A, l, u; ...) -> (x, flag)``.

    ``linearSolverMode`` (SolveQuadraticProgram.jl:11): ``modeDirect`` = a factorisation on the device -- the sparse L D L' of the
    KKT matrix when both matrices are scipy-sparse (what the reference's direct branch does, :168-172), the dense reduced Cholesky
    otherwise; ``modeItertaive`` = matrix-free CG (:153-157); ``modeAuto`` = the reference's size / density rule (see
    ``AutoLinearSolverMode``).  Note that the rule was tuned for a CPU: it sends every problem with more than 5000 rows -- BASELINE's
    dense n = 4096, m = 8192 included -- to CG; pass ``modeDirect`` (or a plugin pair to ``SolveQuadraticProgramInplace``) to keep
    such a problem on the factorisation path."""
    mode = LinearSolverMode(linearSolverMode)
    n = mP.shape[0]
    if mode == LinearSolverMode.modeAuto:
        mode = AutoLinearSolverMode(mP, mA)
    if mode == LinearSolverMode.modeDirect:
        pair = (HipLdlInit, HipLdl) if (sp.issparse(mP) and sp.issparse(mA)) else (HipCholInit, HipChol)
    else:
        pair = (HipCgInit, HipCg)
    vX = np.zeros(n)
    flag = SolveQuadraticProgramInplace(vX, mP, vQ, mA, vL, vU, *pair, **kw)
    return vX, flag
