"""The case table of tests/test_gpu_width_bands.py (GPU) and tests/test_width_bands_cpu.py (CPU guards): one case per width band of the dense loop's
two launches -- the fused pass k_apass<T, TH, KC, R, CHECK, MODE> and the fused sweep -- in both types, with the structured fp64 reference the GPU
runs are held to.  Plain importable helper, no device needed.

The bands.  NP = roundup(n, 64); VN = 2 (fp64) / 4 (fp32); a chunk is 512 * VN columns (1024 / 2048), chunk k of a thread starts at
tid * VN + k * CHUNK and is masked by c < NP.  The handle reports ``sweepVariant`` and ``trsvBlock`` only (asserted on the GPU); the rest is read
off the dispatch code, restated below as ``pass_route`` / ``sweep_route`` / ``proxqp_route`` / ``pick_nb`` / ``apass_plan`` and asserted against
every case's claim by the CPU guards:
  pass     k_pass.hip apass: pass_threads_for -> 1024 threads beyond 8 * 512 * VN, else 512; apass_th: kc = ceil(NP / (TH * VN)), KC = 1 / 2 / 4 / 8 by
           ``kc <= 1 / <= 2 / <= 4 / else``; (R plain, R check) = (4,4) (4,4) (4,2) (2,1) at 512 threads, (4,4) (4,2) (2,1) (1,1) at 1024.
  sweep    dense_chol.h chol_sweep_variant: 2 when sweep_fused_supported (1024 <= NP <= 16 * 512 * VN), else 3 (two gemv sweeps; NP < 1024).
           k_trsv.hip sweep_fused: sweep_wave_covers (NP <= 64 * VN * 8) -> k_sweep_fused_wave<KCW 4> up to 64 * VN * 4, else <KCW 8, single buffer>;
           otherwise kc = ceil(NP / (512 * VN)): ``kc > 8`` -> k_sweep_fused<KC 12 | 16, RB 1, single buffer>, else KC = 1 / 2 / 4 / 8 by
           ``kc <= 1 / <= 2 / <= 4 / else`` with the row block RB = sweep_rb_for(kc) on the real chunk count, ``kc >= 4 ? 1 : (kc == 2 ? 2 : 4)``:
           kc 1 -> 4, 2 -> 2, 3 -> 4, >= 4 -> 1.  So <KC 4> runs as <4, 4> with three chunks (the entry cases fp64 2052, fp32 4100) and as <4, 1>
           with four (the last-chunk cases fp64 3076, fp32 6148); <KC 2> is <2, 2>, <KC 8> is <8, 1>.
  proxqp   k_pass_pq.hip apass_proxqp: MODE 1, 512 threads, KC = 1 / 2 / 4 / 8 and R = 4 / 4 / 4 / 2 by the same ``kc``; refused beyond 8 * 512 * VN.
           The report does not say whether the loop ran fused, so that is not asserted: qps_proxqp.hip takes the MODE 1 pass when loopVariant != 1 and
           apass_proxqp_slabs(NP, MP) > 0, which holds for all six cases (NP <= 8 * 512 * VN); their solve is the sweep of the ADMM case of the same NP.
  trsv     dense_chol.h pick_nb(0, NP): 32768 while the fused sweep covers NP, halved while half of it still covers NP.

Rows.  m = 2130 (ProxQP: me + mi = 701 + 1429, the equality / inequality boundary inside a row tile of every R): MP = roundup(2130, 64) = 2176;
k_pass.hip apass_plan with count = 1: target = 256 workgroups, rpw = ceil(2176 / 256) = 9 rounded up to a multiple of 4 = 12 rows per workgroup,
G = ceil(2176 / 12) = 182 workgroups, the last one holds 2176 - 181 * 12 = 4 rows (ragged), and workgroup 177 holds the last real row (2129) in
the middle of its second tile.  12 rows are 3 / 6 / 12 tiles of the plain variants (R = 4 / 2 / 1): buffer A, buffer B and a reload of A everywhere.

The problem family (``family``).  P = diag(d) + U U', d in [0.5, 1.5], U n x 8 ~ N(0, 1/n); A m x n ~ N(0, 1/n); q ~ N(0, 1); l, u = -/+ 1.05 (0.5 + U(0, 1)),
which leaves about a third of the rows at a bound after 20 iterations (asserted on the CPU); x0 ~ 0.3 N(0, 1).  Every case slices the same base
draw, so the cases of a run share their random data.  ``B`` is the first column of the top chunk the case uses; the columns of A and the rows of U
at index >= B are scaled by WEIGHT = 30 so that the few real columns only that chunk touches carry a visible share of every row dot and of x.  The
device gets P and A as ordinary dense Fortran-ordered matrices (P exactly symmetric: U U' comes from one symmetric rank-k update).  The reference
never forms P: M = P + σI + ρA'A = D~ + W W', W = [U, sqrt(ρ) A'], is solved through the (8 + m)-square capacitance matrix (Woodbury), and
P x = d o x + U (U'x).  ``admm_loop`` restates SolveQuadraticProgram.jl:45-71 with the residuals of :85-89, ``proxqp_loop`` ProxQP.jl:208-249 and
:252-298, each over a backend that supplies the four products: ``Structured`` (fp64, Woodbury, with the three bug models of the CPU guards) or
``DenseF32`` (the fp32 emulation: the same loop in numpy.float32 over a dense float32 Cholesky factor).

Cases ("entry": the first n of a band, ragged inside its 64-pad -- a dispatch off-by-one, the mask of a barely used chunk; "last": 4 real columns
in the last chunk the instantiation has -- chunk addressing with every chunk live).  NP, B, the instantiations: ``CASES`` / ``PQ_CASES`` below.
Not covered: fp32 beyond n = 24576 (sweep KC 16 in fp32; its host matrix alone is 4.9 GB, and the fp64 KC 16 cases run the same template code);
the premultiplied blocked sweep (variant 5).  The batched passes (KC 1 to 8), the batched sweeps and the batched block-phase sweep (variant 1) have
their own table, tests/batch_band_cases.py, which lists what is still uncovered in a batch (the 1024-thread pass among it).  The polishing pass (MODE 2, apass_kkt: the same bands) has its own table,
tests/polish_band_cases.py: it needs neither a converged state nor MINRES iteration counts, because its active sets are the signs of a chosen y.

Bounds.  fp64: TOL["f64"] of loop_param_cases.py (ProxQP: the bounds of test_iterates_and_report_match_oracle).  fp32: 100 x the error of the
fp32 emulation against the fp64 reference, recorded once per case in EMU_F32 (the CPU guards repeat the emulation for n <= 4100 only; the larger
ones cost tens of seconds of CPU factorisation), never looser than TOL["f32"].  The factor 100 is a margin for the device's explicit inverse and
other summation order.  The rule holds for every compared quantity, the two residuals included: each has its own recorded figure.

Measured on an MI355X (printed before every assertion, run with -s; "a against b" = largest figure of the cases against its bound; wall = the whole
test, family, reference and handle included).  No case came near its bound and none needed the evidence procedure for a raised fp32 bound.
  ADMM fp64    n = 2052 / 3076 / 4100 / 7172 / 12292 / 15364: x 2.9e-15 against 1e-9, z 1.8e-14 against 1e-9, y 1.3e-15 against 1e-8, resPrim 4.6e-15 and
               resDual 8.4e-14 against 1e-9; adaptive run at 2052 (one refactor at iteration 11): 2.8e-14 on the iterates, 2.3e-13 on resDual.
               Wall 0.9 (both runs) / 0.3 / 0.3 / 0.5 / 0.8 / 1.3 s.
  ADMM fp32    n, then x / z / y measured against bound (100 x the emulation's own error), then the wall time:
               1092   5.6e-7 / 1.5e-6 / 3.2e-7 against 6.1e-5 / 1.4e-4 / 2.2e-5   0.2 s        2052   4.8e-7 / 3.2e-6 / 2.4e-7 against 5.1e-5 / 1.9e-4 / 1.8e-5   0.2 s
               4100   8.5e-7 / 3.2e-6 / 3.2e-7 against 5.2e-5 / 2.9e-4 / 3.5e-5   0.3 s        6148   5.7e-7 / 1.0e-6 / 3.1e-7 against 5.8e-5 / 4.5e-4 / 3.6e-5   0.4 s
               8196   9.6e-7 / 2.3e-6 / 5.3e-7 against 6.4e-5 / 3.8e-4 / 3.4e-5   0.6 s        14340  1.4e-6 / 4.3e-6 / 4.6e-7 against 7.7e-5 / 5.7e-4 / 4.5e-5   1.0 s
               16388  1.1e-6 / 3.4e-6 / 5.8e-7 against 8.7e-5 / 3.7e-4 / 4.6e-5   1.2 s
               residuals: resPrim <= 4.1e-7 against 2.0e-5 ... 1.6e-4 (100 x each case's own figure), resDual <= 9.8e-6 against 4.9e-5 (n = 14340) ... 6.7e-4.
               The device stays within 2 x the emulation's own error on the vectors.
  ProxQP fp64  n = 2052 / 3076 / 7172: x 2.3e-15 against 1e-8, y 9.0e-16 and z 8.9e-16 against 1e-7, s 6.2e-15 against 1e-8, resPrim 2.7e-15 against
               1e-8, resDual 2.2e-13 against 1e-7; loopVariant 1 at 3076 the same to the last digit shown but x 1.3e-15, s 3.3e-15; adaptive run at 2052
               (ρ 0.1 -> 0.279 at the first check): 1.0e-13 on the state, 1.3e-12 on resDual.  Wall 0.5 (both runs) / 0.3 (both loops) / 0.5 s.
  ProxQP fp32  n, then x / y / z / s measured against bound, then the wall time:
               2052   4.1e-7 / 3.0e-7 / 2.7e-7 / 8.7e-7 against 5.1e-5 / 2.4e-5 / 2.7e-5 / 5.6e-5   0.2 s
               6148   5.8e-7 / 2.2e-7 / 3.0e-7 / 2.7e-7 against 3.8e-5 / 1.9e-5 / 3.7e-5 / 6.6e-5   0.5 s
               14340  1.1e-6 / 3.5e-7 / 3.1e-7 / 3.2e-7 against 5.1e-5 / 2.6e-5 / 3.0e-5 / 8.1e-5   1.0 s
               residuals: resPrim <= 8.1e-7 against 5.4e-5 ... 5.9e-5, resDual <= 5.0e-6 against 7.4e-5 (n = 6148) ... 6.1e-4."""
import math
from collections import namedtuple

import numpy as np
import scipy.linalg as sla

from loop_param_cases import TOL
from quadraticprogramsolver_amd.generator import make_rng

WEIGHT = 30.0
M_ROWS = 2130
PQ_ME, PQ_MI = 701, 1429
RHO, SIGMA, ALPHA = 0.1, 1e-6, 1.6                                     # ADMM: ρ of the issue, σ and α of the reference signature
PQ_RHO, PQ_SIGMA, PQ_TAU = 0.1, 1e-2, 10.0                             # ProxQP: σ and τ of ProxQP.jl:118; ρ = 0.1 keeps M as well conditioned as the ADMM one
K, PERIOD = 20, 10                                                     # the last iteration is a check
N_MAX = 16388
VN = {"f64": 2, "f32": 4}

# kind: entry / last; chunk: columns per chunk of the kernel ``B`` refers to; pass_: (TH, KC, R plain, R check); sweep: ("gemv",) / ("wave", KCW) / ("fused", KC, RB)
Case = namedtuple("Case", "dtype n kind NP B chunk pass_ sweep nb")
CASES = [
    Case("f64", 2052, "entry", 2112, 2048, 1024, (512, 4, 4, 2), ("fused", 4, 4), 4096),             # three chunks: RB 4
    Case("f64", 3076, "last", 3136, 3072, 1024, (512, 4, 4, 2), ("fused", 4, 1), 4096),
    Case("f64", 4100, "entry", 4160, 4096, 1024, (512, 8, 2, 1), ("fused", 8, 1), 8192),
    Case("f64", 7172, "last", 7232, 7168, 1024, (512, 8, 2, 1), ("fused", 8, 1), 8192),
    Case("f64", 12292, "entry", 12352, 12288, 1024, (1024, 8, 1, 1), ("fused", 16, 1), 16384),
    Case("f64", 15364, "last", 15424, 15360, 1024, (1024, 8, 1, 1), ("fused", 16, 1), 16384),    # chunk 7 of the pass starts at 14336: B lies inside it
    Case("f32", 1092, "entry", 1152, 1024, 256, (512, 1, 4, 4), ("wave", 8), 2048),               # wave chunk 64 * VN = 256: chunk 4 of 8
    Case("f32", 2052, "entry", 2112, 2048, 2048, (512, 2, 4, 4), ("fused", 2, 2), 4096),
    Case("f32", 4100, "entry", 4160, 4096, 2048, (512, 4, 4, 2), ("fused", 4, 4), 8192),             # three chunks: RB 4
    Case("f32", 6148, "last", 6208, 6144, 2048, (512, 4, 4, 2), ("fused", 4, 1), 8192),
    Case("f32", 8196, "entry", 8256, 8192, 2048, (512, 8, 2, 1), ("fused", 8, 1), 16384),
    Case("f32", 14340, "last", 14400, 14336, 2048, (512, 8, 2, 1), ("fused", 8, 1), 16384),
    Case("f32", 16388, "entry", 16448, 16384, 2048, (1024, 8, 1, 1), ("fused", 12, 1), 32768),    # chunk 4 of the 4096-column pass chunks starts at 16384 too
]
# ProxQP (MODE 1): pass_ = (512, KC, R, R); the sweep is the one of the ADMM case of the same NP
PQ_CASES = [
    Case("f64", 2052, "entry", 2112, 2048, 1024, (512, 4, 4, 4), ("fused", 4, 4), 4096),
    Case("f64", 3076, "last", 3136, 3072, 1024, (512, 4, 4, 4), ("fused", 4, 1), 4096),
    Case("f64", 7172, "last", 7232, 7168, 1024, (512, 8, 2, 2), ("fused", 8, 1), 8192),
    Case("f32", 2052, "entry", 2112, 2048, 2048, (512, 2, 4, 4), ("fused", 2, 2), 4096),
    Case("f32", 6148, "last", 6208, 6144, 2048, (512, 4, 4, 4), ("fused", 4, 1), 8192),
    Case("f32", 14340, "last", 14400, 14336, 2048, (512, 8, 2, 2), ("fused", 8, 1), 16384),
]
ADAPTIVE_N = 2052                                                      # fp64: one adptΡ = True run of each solver at this n
ADMM_FCTR = 2.0                                                        # fctrΡ of the adaptive ADMM run: the proposal of the first check must cross it (CPU guard)
PQ_BOTH_VARIANTS_N = 3076                                              # fp64 ProxQP case that also runs loopVariant = 1
PQ_TOL64 = dict(x=1e-8, y=1e-7, z=1e-7, s=1e-8, resPrim=1e-8, resDual=1e-7)   # test_iterates_and_report_match_oracle
PQ_TOL32 = dict(x=2e-3, y=2e-2, z=2e-2, s=2e-3, resPrim=2e-3, resDual=2e-2)   # test_fp32_handles_track_the_fp64_restatement (residuals: as TOL["f32"])

# Error of the fp32 emulation against the fp64 reference (``emulation_error``), recorded on the CPU once per case.
EMU_F32 = {
    ("admm", 1092): dict(x=6.05e-07, z=1.39e-06, y=2.19e-07, resPrim=2.11e-07, resDual=6.70e-06),
    ("admm", 2052): dict(x=5.08e-07, z=1.89e-06, y=1.76e-07, resPrim=3.04e-07, resDual=1.23e-06),
    ("pq", 2052): dict(x=5.12e-07, y=2.40e-07, z=2.65e-07, s=5.62e-07, resPrim=5.38e-07, resDual=6.13e-06),
    ("admm", 4100): dict(x=5.16e-07, z=2.86e-06, y=3.47e-07, resPrim=2.05e-07, resDual=4.09e-06),
    ("admm", 6148): dict(x=5.84e-07, z=4.50e-06, y=3.57e-07, resPrim=1.61e-06, resDual=3.01e-06),
    ("pq", 6148): dict(x=3.82e-07, y=1.95e-07, z=3.73e-07, s=6.63e-07, resPrim=5.71e-07, resDual=7.37e-07),
    ("admm", 8196): dict(x=6.40e-07, z=3.80e-06, y=3.37e-07, resPrim=2.63e-07, resDual=2.41e-06),
    ("admm", 14340): dict(x=7.67e-07, z=5.69e-06, y=4.49e-07, resPrim=1.09e-06, resDual=4.89e-07),
    ("pq", 14340): dict(x=5.06e-07, y=2.57e-07, z=2.97e-07, s=8.09e-07, resPrim=5.88e-07, resDual=5.10e-06),
    ("admm", 16388): dict(x=8.71e-07, z=3.69e-06, y=4.62e-07, resPrim=1.04e-06, resDual=3.35e-06),
}


def case_id(c):
    return f"{c.dtype}-n{c.n}"


# ---------------------------------------------------------------------------------------------------------------------
# The dispatch code, restated (file and function in the docstring above)
# ---------------------------------------------------------------------------------------------------------------------
def roundup(a, b):
    return (a + b - 1) // b * b


def pass_route(dtype, NP):
    vn = VN[dtype]
    if NP > 8 * 1024 * vn:
        return None
    th = 1024 if NP > 8 * 512 * vn else 512
    kc = -(-NP // (th * vn))
    table = {512: ((1, 4, 4), (2, 4, 4), (4, 4, 2), (8, 2, 1)), 1024: ((1, 4, 4), (2, 4, 2), (4, 2, 1), (8, 1, 1))}[th]
    return (th,) + table[0 if kc <= 1 else 1 if kc <= 2 else 2 if kc <= 4 else 3]


def proxqp_route(dtype, NP):
    vn = VN[dtype]
    if NP > 8 * 512 * vn:
        return None
    kc = -(-NP // (512 * vn))
    return (512,) + ((1, 4, 4), (2, 4, 4), (4, 4, 4), (8, 2, 2))[0 if kc <= 1 else 1 if kc <= 2 else 2 if kc <= 4 else 3]


def sweep_fused_supported(dtype, NP):
    return 1024 <= NP <= 16 * 512 * VN[dtype]


def sweep_rb_for(kc):
    return 1 if kc >= 4 else 2 if kc == 2 else 4


def sweep_route(dtype, NP):
    vn = VN[dtype]
    if not sweep_fused_supported(dtype, NP):
        return ("gemv",)
    if NP <= 64 * vn * 8:
        return ("wave", 4 if NP <= 64 * vn * 4 else 8)
    kc = -(-NP // (512 * vn))
    if kc > 8:
        return ("fused", 12 if kc <= 12 else 16, 1)
    return ("fused", 1 if kc <= 1 else 2 if kc <= 2 else 4 if kc <= 4 else 8, sweep_rb_for(kc))


def sweep_variant(dtype, NP):
    return 2 if sweep_fused_supported(dtype, NP) else 3


def pick_nb(dtype, NP):
    nb = 32768 if sweep_fused_supported(dtype, NP) else 4096
    while nb > 64 and nb // 2 >= NP:
        nb //= 2
    return nb


def apass_plan(MP):
    """(rows per workgroup, workgroups) of a single QP."""
    rpw = roundup(-(-MP // 256), 4)
    return rpw, -(-MP // rpw)


# ---------------------------------------------------------------------------------------------------------------------
# The family
# ---------------------------------------------------------------------------------------------------------------------
_base = {}


def _base_draw():
    if not _base:
        rng = make_rng(2718, 1)
        _base.update(d=0.5 + rng.random(N_MAX), U=rng.standard_normal((N_MAX, 8)), A=np.asfortranarray(rng.standard_normal((N_MAX, M_ROWS)).T),
                     q=rng.standard_normal(N_MAX), x0=0.3 * rng.standard_normal(N_MAX), lo=0.5 + rng.random(M_ROWS), hi=0.5 + rng.random(M_ROWS),
                     xf=rng.standard_normal(N_MAX), margin=0.3 * np.abs(rng.standard_normal(M_ROWS)) + 0.3, y0=0.1 * rng.standard_normal(M_ROWS))
    return _base


def _member_draw(member, n, m):
    """The draw of member ``member`` of a batch (tests/batch_band_cases.py): the same distributions from that member's own stream, sized to the member."""
    rng = make_rng(2718, 2 + member)
    return dict(d=0.5 + rng.random(n), U=rng.standard_normal((n, 8)), A=np.asfortranarray(rng.standard_normal((n, m)).T), q=rng.standard_normal(n),
                x0=0.3 * rng.standard_normal(n), lo=0.5 + rng.random(m), hi=0.5 + rng.random(m))


class Family:
    """One member: d, U (weighted), A (m x n, Fortran order, weighted), q, l, u, x0, and for ProxQP b, dd, the explicit start (x0, y0, z0, s0).
    ``member`` (optional, ADMM only): QP number ``member`` of a batch, every array from its own stream, A times ``scale``, l and u times ``tight``; None is the base draw."""

    def __init__(self, n, B, m=M_ROWS, weight=WEIGHT, me=None, member=None, scale=1.0, tight=1.0):
        b = _base_draw() if member is None else _member_draw(member, n, m)
        assert (member is not None and me is None) or (n <= N_MAX and m <= M_ROWS and scale == tight == 1.0)
        assert 0 < B < n
        self.n, self.m, self.B, self.member, self.scale = n, m, B, member, scale
        wcol = np.where(np.arange(n) >= B, weight, 1.0)
        self.d = b["d"][:n].copy()
        self.U = b["U"][:n] * (wcol / math.sqrt(n))[:, None]
        self.A = np.asfortranarray(b["A"][:m, :n] * (wcol / math.sqrt(n))[None, :])
        if member is not None:
            self.A *= scale
        self.q, self.x0 = b["q"][:n].copy(), b["x0"][:n].copy()
        self.l, self.u = -1.05 * b["lo"][:m], 1.05 * b["hi"][:m]
        if member is not None:
            self.l, self.u = tight * self.l, tight * self.u
        self.me = me
        if me is not None:                                              # ProxQP: G = [A; C] = the rows of self.A, b = A xf, d = C xf + margin
            xf = b["xf"][:n] / wcol
            g = self.A @ xf
            self.b, self.dd = g[:me].copy(), g[me:] + b["margin"][:m - me]
            self.y0, self.z0 = b["y0"][:me].copy(), np.abs(b["y0"][me:m])
            self.s0 = np.maximum(self.dd - self.A[me:] @ self.x0, 0.0)
        self._cache = {}

    def dense_P(self):
        """P as the device gets it: Fortran-ordered, exactly symmetric (the rank-k update fills both triangles from one computation)."""
        P = self.U @ self.U.T
        P[np.diag_indices_from(P)] += self.d
        return P.T


_families = {}


def family(case, pq=False):
    """The family member of a case, cached; treat as read-only."""
    key = (case.n, case.B, pq)
    if key not in _families:
        _families.clear()                                               # one member at a time: the largest holds 0.6 GB
        _families[key] = Family(case.n, case.B, me=PQ_ME if pq else None)
    return _families[key]


def small_family(pq=False):
    """The small member the structured references are checked on against the project's oracles: n = 300, m = 200, B = 296 (4 weighted columns, as in the cases)."""
    return Family(300, 296, m=200, me=70 if pq else None)


# ---------------------------------------------------------------------------------------------------------------------
# Backends: the four products of a loop.  bug: 0 none; 1 columns >= B ignored in the row dot; 2 columns >= B ignored in the column accumulation;
# 3 entries >= B of the right-hand side ignored by the solve.
# ---------------------------------------------------------------------------------------------------------------------
class Structured:
    dtype = np.float64

    def __init__(self, f, bug=0):
        self.f, self.bug = f, bug

    def factor(self, rho, sigma):
        key = (rho, sigma)
        if key not in self.f._cache:                                    # shared by the bug models of a case
            f = self.f
            dt = f.d + sigma
            W = np.hstack([f.U, math.sqrt(rho) * f.A.T])
            Wd = W / dt[:, None]
            cap = W.T @ Wd
            cap[np.diag_indices_from(cap)] += 1.0
            self.f._cache.clear()
            self.f._cache[key] = (dt, W, Wd, sla.cho_factor(cap, lower=True, overwrite_a=True))
        self.fac = self.f._cache[key]

    def solve(self, r):
        dt, W, Wd, c = self.fac
        if self.bug == 3:
            r = r.copy(); r[self.f.B:] = 0.0
        t = r / dt
        return t - Wd @ sla.cho_solve(c, W.T @ t)

    def Ax(self, x, rows=slice(None), check=False):
        B = self.f.B
        return self.f.A[rows, :B] @ x[:B] if self.bug == 1 and not check else self.f.A[rows] @ x

    def Atw(self, w, rows=slice(None), check=False):
        r = self.f.A[rows].T @ w
        if self.bug == 2 and not check:
            r[self.f.B:] = 0.0
        return r

    def Px(self, x):
        return self.f.d * x + self.f.U @ (self.f.U.T @ x)


class DenseF32:
    """The fp32 emulation: every array and every scalar in numpy.float32, M factorised by a dense float32 Cholesky."""
    dtype = np.float32

    def __init__(self, f):
        self.f = f
        self.A = f.A.astype(np.float32)
        U = f.U.astype(np.float32)
        self.P = U @ U.T
        self.P[np.diag_indices_from(self.P)] += f.d.astype(np.float32)
        self.AA = self.A.T @ self.A

    def factor(self, rho, sigma):
        M = self.P + np.float32(rho) * self.AA
        M[np.diag_indices_from(M)] += np.float32(sigma)
        self.c = sla.cho_factor(M, lower=True, overwrite_a=True, check_finite=False)
        assert self.c[0].dtype == np.float32

    def solve(self, r):
        return sla.cho_solve(self.c, r, check_finite=False)

    def Ax(self, x, rows=slice(None), check=False):
        return self.A[rows] @ x

    def Atw(self, w, rows=slice(None), check=False):
        return self.A[rows].T @ w

    def Px(self, x):
        return self.P @ x


def _ninf(v):
    return float(np.abs(v).max()) if v.size else 0.0


def admm_loop(be, numIterations=K, numItrConv=PERIOD, rho=RHO, sigma=SIGMA, alpha=ALPHA, adpt=False, fctr=5.0):
    """SolveQuadraticProgram.jl:45-71 with ϵAbs = ϵRel = 0 (no stop) and the residuals of :85-89, in the arithmetic of ``be``.  Returns a dict."""
    T, f = be.dtype, be.f
    q, l, u = f.q.astype(T), f.l.astype(T), f.u.astype(T)
    x, z, y = f.x0.astype(T), np.zeros(f.m, T), np.zeros(f.m, T)
    rho_prop, nref, res, norms = rho, 0, (math.nan, math.nan), None
    be.factor(rho, sigma)                                               # :36
    for ii in range(1, numIterations + 1):                              # :45
        if adpt and (rho_prop * fctr < rho or rho_prop > fctr * rho):   # :47-51
            rho = rho_prop; nref += 1
            be.factor(rho, sigma)
        a, a1, r, r1, s = T(alpha), T(1) - T(alpha), T(rho), T(1) / T(rho), T(sigma)
        xx = be.solve(s * x - q + be.Atw(r * z - y))                    # LinearSystemSolvers.jl:134-137
        zz = be.Ax(xx)                                                  # :139
        xp, zp = x, z
        x = a * xx + a1 * x                                             # :56-57
        z = np.clip(a * zz + a1 * zp + r1 * y, l, u)                    # :59-60
        y = y + r * (a * zz + a1 * zp - z)                              # :61
        if ii % numItrConv == 0:                                        # :63
            Ax, Px, Aty = be.Ax(x, check=True), be.Px(x), be.Atw(y, check=True)
            res = (_ninf(Ax - z), _ninf(Px + q + Aty))                  # :85-86
            norms = (max(_ninf(Ax), _ninf(z)), max(_ninf(Px), _ninf(Aty), _ninf(q)))   # :88-89
            if adpt:                                                    # :92-96
                rho_prop = float(np.clip(rho * math.sqrt(res[0] * norms[1] / (res[1] * norms[0])), 1e-3, 1e6))
    return dict(x=x.astype(np.float64), z=z.astype(np.float64), y=y.astype(np.float64), resPrim=res[0], resDual=res[1], iterations=numIterations,
                rhoFinal=rho, rhoProposed=rho_prop, numRefactor=nref, maxNormPrim=norms[0], maxNormDual=norms[1], active=float(np.mean((z == l) | (z == u))))


def proxqp_loop(be, numIterations=K, numItrConv=PERIOD, rho=PQ_RHO, sigma=PQ_SIGMA, adpt=False, tau=PQ_TAU):
    """ProxQP.jl:118-173 with CalculateRhs! / UpdateX,S,Y,Z! (:208-249) and CheckConvergence! (:252-298) at ϵAbs = ϵRel = 0, from the explicit
    state of the family, in the arithmetic of ``be``.  Returns a dict with the state and the report."""
    T, f = be.dtype, be.f
    me = f.me
    E, I = slice(0, me), slice(me, f.m)
    q, b, d = f.q.astype(T), f.b.astype(T), f.dd.astype(T)
    x, y, z, s = f.x0.astype(T), f.y0.astype(T), f.z0.astype(T), f.s0.astype(T)
    rho_rep, res, nupd, mp, md, first = rho, (math.inf, math.inf), 0, math.nan, math.nan, 0
    be.factor(rho, sigma)                                               # :131
    for ii in range(1, numIterations + 1):                              # :135
        r, r1 = T(rho), T(1) / T(rho)
        rhs = T(sigma) * x - q + be.Atw(np.concatenate([r * b - y, r * (d - s) - z]))   # :211-216
        x = be.solve(rhs)                                               # :224
        gx = be.Ax(x)
        ax, cx = gx[E], gx[I]
        s = np.maximum(d - r1 * z - cx, T(0))                           # :230-232
        y = y - r * b + r * ax                                          # :238-239
        z = np.maximum(z + r * (s - d) + r * cx, T(0))                  # :246-248
        if ii % numItrConv == 0:                                        # :151
            X1, X2, X3 = be.Px(x), be.Atw(y, E, check=True), be.Atw(z, I, check=True)   # :261-263
            Bb, Db = be.Ax(x, E, check=True), be.Ax(x, I, check=True)   # :264-265
            res = (max(_ninf(Bb - b), _ninf(Db - d + s)), _ninf(X1 + X2 + X3 + q))       # :266-267
            mp, md = max(_ninf(Bb), _ninf(b), _ninf(Db), _ninf(d), _ninf(s)), max(_ninf(X1), _ninf(X2), _ninf(X3), _ninf(q))   # :269-270
            if adpt:                                                    # :277-286
                ratio = res[0] * md / (res[1] * mp)
                if ratio > tau or 1.0 / ratio > tau:
                    rho = float(np.clip(rho * math.sqrt(math.sqrt(ratio)), 1e-5, 1e5))
                    rho_rep = rho; nupd += 1; first = first or ii
                    be.factor(rho, sigma)                               # :159-165
    return dict(x=x.astype(np.float64), y=y.astype(np.float64), z=z.astype(np.float64), s=s.astype(np.float64), resPrim=res[0], resDual=res[1],
                rho=rho_rep, updates=nupd, firstUpdate=first, maxNormPrim=mp, maxNormDual=md, active=float(np.mean(s == 0)))


# ---------------------------------------------------------------------------------------------------------------------
# Errors and bounds
# ---------------------------------------------------------------------------------------------------------------------
def rel(a, b):
    return np.abs(a - b).max() / max(1.0, np.abs(b).max()) if b.size else 0.0


ADMM_KEYS = ("x", "z", "y", "resPrim", "resDual")
PQ_KEYS = ("x", "y", "z", "s", "resPrim", "resDual")


def errors(got, ref, keys):
    """Relative max-norm error of every vector, |a - b| / max(1, |b|) of every scalar: the measure of the existing loop tests."""
    return {k: (rel(got[k], ref[k]) if isinstance(ref[k], np.ndarray) else abs(got[k] - ref[k]) / max(1.0, abs(ref[k]))) for k in keys}


def emulation_error(case, pq=False):
    """The fp32 emulation of a case against its fp64 reference: the figures recorded in EMU_F32."""
    f = family(case, pq)
    loop, keys = (proxqp_loop, PQ_KEYS) if pq else (admm_loop, ADMM_KEYS)
    return errors(loop(DenseF32(f)), loop(Structured(f)), keys)


def bounds(case, pq=False):
    """The bound of every compared quantity of a case."""
    cap = (PQ_TOL32 if pq else TOL["f32"]) if case.dtype == "f32" else (PQ_TOL64 if pq else TOL["f64"])
    if case.dtype == "f64":
        return dict(cap)
    emu = EMU_F32[("pq" if pq else "admm", case.n)]
    return {k: min(100.0 * emu[k], cap[k]) for k in cap}
