"""The case table of tests/test_gpu_polish_bands.py (GPU) and tests/test_polish_bands_cpu.py (CPU guards): one case per width band of the polishing
step's masked KKT product -- k_pass_pq.hip apass_kkt, MODE 2 of k_apass<T, 512, KC, R, false, 2> -- in both types, the two-GEMV fallback at its natural
size, and the references the GPU runs are held to.  Plain importable helper, no device needed.

Why no ADMM state is needed.  qps_polish takes any (x, y); the active sets are the SIGNS of y (SolveQuadraticProgram.m:293-294), which the test chooses;
the iteration starts from t = 0 (:307), so x only has to be replaced.  With flag 0 the polished x solves the reduced KKT system  [P A_act'; A_act 0]
[x; λ] = [-q; bound]  whatever MINRES did on the way, so the reference is a direct solve.  A one-sided error in the product breaks the symmetry MINRES
relies on and shows as flag != 0; a symmetric one shows as a wrong x.

The bands (``polish_route``, asserted against every case's claim on the CPU).  qps_polish.hip polish_dense takes the fused product iff
apass_proxqp_slabs > 0, i.e. NP <= 8 * 512 * VN (VN = 2 fp64 / 4 fp32); apass_kkt: kc = ceil(NP / (512 * VN)), (KC, R) = (1, 4) (2, 4) (4, 4) (8, 2) by
``kc <= 1 / <= 2 / <= 4 / else``.  Beyond that the product is gemv_rows (A v_x), k_pol_maskrow, gemv_cols_partial and colsum.  "entry": the first n of a
band, ragged inside its 64-pad; "last": 4 real columns in the last chunk the instantiation has.  ``B`` is the first column of the top used chunk.
KC 1 runs in tests/test_gpu_polish.py (n <= 1100 in fp64, n = 64 in fp32) and in the tall case below.

Inputs.  Family(n, B) of width_band_cases.py: P = diag(d) + U U', m = 2130 rows (MP = 2176: 12 rows per workgroup, 182 workgroups, the last one ragged, the
last real row in workgroup 177), columns >= B weighted by 30.  The multiplier is ``y_pattern``: a multiplicative hash of the row index makes a quarter of
the rows lower-active and an eighth upper-active with magnitudes 0.25 * 2^[0, 5] (fp32 keeps every sign), then row 0 and row m - 1 are active, workgroup 88
(rows 1056-1067) is all inactive, workgroup 89 all active with alternating sign, rows 479 | 480 are active across a workgroup boundary and rows 493-496
across a tile boundary of R = 2 only (493 | 494) and of R = 4 and R = 2 (495 | 496): 536 lower and 271 upper rows.  x0 is the family's.

Runs.  A: the defaults δ = 1e-6, numItrPolish = 10, ϵMinres = 1e-10 (fp32: numItrPolish = 3, ϵMinres = 1e-3, the figure of test_polish_other_product_paths);
flag 0, numActiveLower / Upper = 536 / 271, x = the direct solve.  B: δ = 1e-2, numItrPolish = 1, the same ϵMinres, against the direct solve of the
regularised system K + δ blkdiag(I, -I): it pins the -δ mask v_λ term, which refinement hides in run A (a dropped δ moves x by 7.4e-3 ... 0.18 there).
Run B is fp64 only: see RUN_B_F32.  numItrMinres is 4 x the largest per-call count of the restated loop (``ITS``).

References.  ``direct``: fp64, never forms P: P^-1 through Woodbury, λ from the Cholesky factor of the Schur complement A_act P^-1 A_act' (run B: P + δI and
+ δI on the Schur complement); equal to np.linalg.solve on the dense K and to polish_oracle_np.Polish to 1e-12 on small_family().  ``refine`` restates
SolveQuadraticProgram.m:307-325 over a product (``StructuredK``: d, U and the active rows of A, with the bug models of the CPU guards; ``DenseK``) and
polish_oracle_np.minres; in numpy.float32 (``minres_t``, a copy of that minres with every vector and scalar in the type) it is the fp32 emulation.  Ten
refinements of the restatement agree with the direct solve to 1.5e-13 (n = 1028) ... 1.6e-15 (n = 8196).

Bounds on |x - x_ref|_inf / max(1, |x_ref|_inf).  fp64 run A: 1e-9, the bound of test_polish_reaches_the_kkt_point_of_the_active_set.  fp64 run B: 100 x the
restatement's own distance from the regularised direct solve (``DIST_B``: 1.6e-10 ... 2.8e-10).  fp32: 100 x the error of the fp32 emulation against the fp64
direct solve (``EMU_F32``: 1.8e-7 ... 2.9e-7), never looser than the 5e-3 of test_polish_other_product_paths; the factor 100 is a margin for the device's
other summation order and its double-precision MINRES scalars, as in the width-band file.

Further cases.  Tall: n = 64, m = 65540 (MP = 65600, N = NP + MP = 65664: 257 partial sums, one beyond a 256-thread trip of sum_partials), dense P, its own
draw of A, 30 active rows with the last row among them (its multiplier lies in the 257th partial; without that row x moves by 3e-2); dense reference.
Batch: count = 3, n = 2044, m = 1000: the loop's plan is 3 x 64 = 192 slabs, one QP's polishing plan 256 (``apass_plan``); the three members differ in
every array; the reference of a QP is ``direct`` on the active sets of the y the batch returns; with m <= n / 2 every active set is nonsingular.
(test_gpu_parity.py has the same slab relation at n = 1100, 3 x 82 against 256, compared with a single-handle polish; here the reference is independent.)  Chained:
fp64 n = 3076, solve(polish=True) against solve followed by polish on the loop's own (x, y).  Nothing left behind: the same fixed-K solve before and
after polishing is bit-identical in x, z, y (fp64 n = 2052 and the batch).

Measured on an MI355X (printed before every assertion, run with -s; wall = the whole test, family, reference and handle included).  No case came near its
bound.  16 tests in 5.8 s (the width-band file: 12 s).
  fp64   n, run A x against 1e-9 (total MINRES iterations of the ten calls), run B x against its bound (iterations), wall:
         1028  1.5e-13 (8089)   2.4e-10 against 2.5e-8 (556)   0.8 s        2052  1.3e-14 (2661)   2.2e-10 against 2.2e-8 (219)   0.2 s
         3076  1.0e-14 (1991)   1.6e-10 against 1.6e-8 (168)   0.3 s        4100  5.9e-15 (1714)   1.8e-10 against 1.8e-8 (143)   0.3 s
         7172  2.0e-15 (1354)   2.8e-10 against 2.8e-8 (115)   0.5 s        8196  1.8e-15 (1299)   2.2e-10 against 2.1e-8 (110)   0.6 s   (fallback)
         The device's run B distance equals the restatement's to two digits, and its per-call counts stay within 2 of it.
  fp32   n, run A x against 100 x the emulation's own error (iterations of the three calls), wall:
         2052  1.7e-7 against 2.6e-5 (451)  0.1 s    4100  2.2e-7 against 2.9e-5 (290)  0.2 s    6148   2.3e-7 against 1.8e-5 (241)  0.2 s
         8196  2.9e-7 against 1.9e-5 (216)  0.3 s    14340 2.8e-7 against 1.9e-5 (172)  0.6 s    16388  3.0e-7 against 1.8e-5 (174)  0.7 s   (fallback)
         The device stays within 1.7 x the emulation's own error.
  tall   fp64 run A 8.2e-16 (880), run B 5.7e-11 against 5.2e-9 (84); fp32 run A 1.1e-7 against 9.0e-6 (192); 0.1 s each.
  batch  polishFlag 0 for the three QPs, x 1.8e-15 / 1.3e-15 / 9.1e-16 against 1e-9 (1529 / 1284 / 1154 iterations; 311 / 259 / 234 active rows; polishing
         moved x by 2.9e-5 / 6.5e-2 / 2.4e-5); z and y unchanged by polishing; the solves before and after bit-identical.  0.2 s.
  chained  polishFlag 0 / 0, polishIterations 2359 / 2359, x bit-identical (560 lower and 494 upper rows, most of them rounding noise of y).  0.3 s."""
import math
from collections import namedtuple

import numpy as np
import scipy.linalg as sla

import width_band_cases as W
from oracle import polish_oracle_np as PO
from quadraticprogramsolver_amd.generator import make_rng

M_ROWS = W.M_ROWS
RPW, WGS = 12, 182                                                     # apass_plan(2176): rows per workgroup, workgroups
QUIET_WG, BUSY_WG = 88, 89                                             # 12 rows all inactive, then 12 rows all active with alternating sign
EDGE_WG = 40                                                           # rows 479 | 480 are active on both sides of a workgroup boundary
TILE_ROWS = (493, 494, 495, 496)                                       # active: 493 | 494 is a tile boundary of R = 2 only, 495 | 496 of R = 4 and R = 2
N_LOWER, N_UPPER = 536, 271                                            # of y_pattern(): 807 of 2130 rows, three eighths
RUN_A = {"f64": dict(numItrPolish=10, δ=1e-6, ϵMinres=1e-10), "f32": dict(numItrPolish=3, δ=1e-6, ϵMinres=1e-3)}
RUN_B = {"f64": dict(numItrPolish=1, δ=1e-2, ϵMinres=1e-10), "f32": dict(numItrPolish=1, δ=1e-2, ϵMinres=1e-3)}
TOL64_A = 1e-9                                                         # test_polish_reaches_the_kkt_point_of_the_active_set
CAP32 = 5e-3                                                           # test_polish_other_product_paths

# route: ("fused", KC, R) of k_apass<T, 512, KC, R, false, 2>, or ("gemv",): k_pol_maskrow + gemv_cols_partial + wide gemv_rows
Case = namedtuple("Case", "dtype n kind NP B route")
CASES = [
    Case("f64", 1028, "entry+last", 1088, 1024, ("fused", 2, 4)),
    Case("f64", 2052, "entry", 2112, 2048, ("fused", 4, 4)),
    Case("f64", 3076, "last", 3136, 3072, ("fused", 4, 4)),
    Case("f64", 4100, "entry", 4160, 4096, ("fused", 8, 2)),
    Case("f64", 7172, "last", 7232, 7168, ("fused", 8, 2)),
    Case("f64", 8196, "fallback", 8256, 8192, ("gemv",)),
    Case("f32", 2052, "entry+last", 2112, 2048, ("fused", 2, 4)),
    Case("f32", 4100, "entry", 4160, 4096, ("fused", 4, 4)),
    Case("f32", 6148, "last", 6208, 6144, ("fused", 4, 4)),
    Case("f32", 8196, "entry", 8256, 8192, ("fused", 8, 2)),
    Case("f32", 14340, "last", 14400, 14336, ("fused", 8, 2)),
    Case("f32", 16388, "fallback", 16448, 16384, ("gemv",)),
]
LEFT_BEHIND_N = 2052                                                   # fp64 fused case that also checks that polishing leaves nothing behind
CHAINED_N = 3076                                                       # fp64: solve(polish=True) against solve, then polish

# Largest per-call MINRES count of the fp64 restatement at the run's own ϵMinres (``restate``); the device runs get 4 x that (``budget``).
ITS = {
    ("f64-n1028", "A"): 1075, ("f64-n1028", "B"): 557, ("f64-n2052", "A"): 363, ("f64-n2052", "B"): 221, ("f64-n3076", "A"): 270, ("f64-n3076", "B"): 169,
    ("f64-n4100", "A"): 232, ("f64-n4100", "B"): 145, ("f64-n7172", "A"): 185, ("f64-n7172", "B"): 115, ("f64-n8196", "A"): 171, ("f64-n8196", "B"): 110,
    ("f32-n2052", "A"): 147, ("f32-n4100", "A"): 92, ("f32-n6148", "A"): 76, ("f32-n8196", "A"): 70, ("f32-n14340", "A"): 57, ("f32-n16388", "A"): 59,
    ("f32-n2052", "B"): 65, ("f32-n4100", "B"): 44, ("f32-n6148", "B"): 40, ("f32-n8196", "B"): 37, ("f32-n14340", "B"): 26, ("f32-n16388", "B"): 26,   # CPU guard only
    ("tall-f64", "A"): 97, ("tall-f64", "B"): 84, ("tall-f32", "A"): 69,
    ("batch", "A"): 449,                                               # every row active, the worst of the three members (the loop's own sets: 206)
    ("chained", "A"): 277,                                             # the active sets of the restated loop's y after K = 20 iterations
}
# Run B, fp64: distance of the restatement (one MINRES call to 1e-10) from the regularised direct solve.
DIST_B = {"f64-n1028": 2.47e-10, "f64-n2052": 2.21e-10, "f64-n3076": 1.63e-10, "f64-n4100": 1.76e-10, "f64-n7172": 2.83e-10, "f64-n8196": 2.07e-10,
          "tall-f64": 5.25e-11}
# Run A, fp32: error of the fp32 emulation (StructuredK / DenseK and minres_t in numpy.float32) against the fp64 direct solve.
EMU_F32 = {("f32-n2052", "A"): 2.60e-07, ("f32-n4100", "A"): 2.91e-07, ("f32-n6148", "A"): 1.82e-07, ("f32-n8196", "A"): 1.88e-07,
           ("f32-n14340", "A"): 1.95e-07, ("f32-n16388", "A"): 1.85e-07, ("tall-f32", "A"): 8.95e-08,
           # run B (one MINRES call to 1e-3: the truncation, not the rounding; not run on the device, see RUN_B_F32)
           ("f32-n2052", "B"): 1.53e-03, ("f32-n4100", "B"): 1.64e-03, ("f32-n6148", "B"): 1.61e-03, ("f32-n8196", "B"): 1.45e-03,
           ("f32-n14340", "B"): 2.05e-03, ("f32-n16388", "B"): 1.86e-03}
# Run B in fp32: nowhere.  One MINRES call to 1e-3 leaves x 1.3e-3 ... 2.1e-3 from the regularised solve (restatement and emulation alike), so the bound
# is the 5e-3 cap, and the dropped δ term moves x by 4e-3 ... 1.9e-2 only: 0.9 ... 3.9 x that bound, not the 10 x the guard asks for (asserted on the CPU).
RUN_B_F32 = ()


def case_id(c):
    return f"{c.dtype}-n{c.n}"


# ---------------------------------------------------------------------------------------------------------------------
# The dispatch code, restated (k_pass_pq.hip apass_kkt, qps_polish.hip polish_dense)
# ---------------------------------------------------------------------------------------------------------------------
def polish_route(dtype, NP):
    vn = W.VN[dtype]
    if NP > 8 * 512 * vn:                                              # apass_proxqp_slabs == 0: the two-GEMV product
        return ("gemv",)
    kc = -(-NP // (512 * vn))
    return ("fused",) + ((1, 4), (2, 4), (4, 4), (8, 2))[0 if kc <= 1 else 1 if kc <= 2 else 2 if kc <= 4 else 3]


def apass_plan(dtype, NP, MP, count=1):
    """k_pass.hip apass_plan: (rows per workgroup, slabs per QP)."""
    vn = W.VN[dtype]
    th = 1024 if NP > 8 * 512 * vn else 512
    total = 1024 if (NP <= th * vn and count > 1) else 256
    target = 1 if count >= total else total // max(count, 1)
    rpw = W.roundup(-(-MP // target), 4)
    return rpw, -(-MP // rpw)


def minres_partials(NP, MP):
    """nb of qps_polish.hip minres_device: the partial sums that sum_partials adds, 256 per trip."""
    return -(-(NP + MP) // 256)


# ---------------------------------------------------------------------------------------------------------------------
# The multiplier patterns
# ---------------------------------------------------------------------------------------------------------------------
def _magnitude(i):
    h = (i.astype(np.uint64) * np.uint64(2654435761) + np.uint64(12345)) % np.uint64(2 ** 32)
    return h.astype(np.float64) / 2.0 ** 32, 0.25 * 2.0 ** (5.0 * ((h >> np.uint64(7)) % np.uint64(1024)).astype(np.float64) / 1023.0)


def y_pattern(m=M_ROWS):
    """The fixed multiplier of the band cases: a quarter of the rows lower-active (y < 0), an eighth upper-active, magnitudes in [0.25, 8], by a
    multiplicative hash of the row index; then the rows the kernel's row plan makes special (constants above)."""
    i = np.arange(m)
    r, mag = _magnitude(i)
    y = np.where(r < 0.25, -mag, np.where(r < 0.375, mag, 0.0))
    alt = np.where(i % 2 == 0, -mag, mag)
    y[0], y[m - 1] = -mag[0], mag[m - 1]
    if m >= (BUSY_WG + 1) * RPW:
        y[QUIET_WG * RPW:(QUIET_WG + 1) * RPW] = 0.0
        y[BUSY_WG * RPW:(BUSY_WG + 1) * RPW] = alt[BUSY_WG * RPW:(BUSY_WG + 1) * RPW]
        edge = [EDGE_WG * RPW - 1, EDGE_WG * RPW] + list(TILE_ROWS)
        y[edge] = alt[edge]
    return y


TALL_N, TALL_M = 64, 65540                                             # MP = 65600, N = NP + MP = 65664, nb = 257: one partial beyond the first trip of sum_partials
TALL_ROWS = sorted({0, 1, 255, 256, 65535, 65536, TALL_M - 1} | {2731 * k + 17 for k in range(1, 24)})


def tall_pattern():
    """30 active rows of the tall case, the last row among them (its multiplier lies in partial 256, the 257th)."""
    i = np.arange(TALL_M)
    _, mag = _magnitude(i)
    y = np.zeros(TALL_M)
    rows = np.array(TALL_ROWS)
    y[rows] = np.where(np.arange(rows.size) % 2 == 0, -mag[rows], mag[rows])
    return y


class Tall:
    """n = 64, m = 65540: dense P = diag(d) + U U', A ~ N(0, 1/n) from its own draw (34 MB), bounds as in the family."""

    def __init__(self):
        rng = make_rng(2718, 2)
        n, m = TALL_N, TALL_M
        self.n, self.m = n, m
        U = rng.standard_normal((n, 8)) / math.sqrt(n)
        P = U @ U.T
        self.P = 0.5 * (P + P.T)                                          # exactly symmetric
        self.P[np.diag_indices(n)] += 0.5 + rng.random(n)
        self.A = np.asfortranarray(rng.standard_normal((n, m)).T / math.sqrt(n))
        self.q, self.x0 = rng.standard_normal(n), 0.3 * rng.standard_normal(n)
        self.l, self.u = -1.05 * (0.5 + rng.random(m)), 1.05 * (0.5 + rng.random(m))


_tall = []


def tall():
    if not _tall:
        _tall.append(Tall())
    return _tall[0]


# ---------------------------------------------------------------------------------------------------------------------
# The batch family: count = 3, n = 2044 (NP = 2048), m = 1000 (MP = 1024)
# ---------------------------------------------------------------------------------------------------------------------
BATCH_COUNT, BATCH_N, BATCH_M, BATCH_B = 3, 2044, 1000, 2040
BATCH_PLAIN = dict(numIterations=20, ϵAbs=0.0, ϵRel=0.0)
BATCH_SOLVE = dict(BATCH_PLAIN, polish=True, ϵMinres=1e-10)


def batch_members():
    """Three members that differ in every array: d shifted, the rows of A rotated, q rotated and scaled, the bounds scaled."""
    out = []
    for b in range(BATCH_COUNT):
        f = W.Family(BATCH_N, BATCH_B, m=BATCH_M)
        f.d = f.d + 0.25 * b
        f.A = np.asfortranarray(np.roll(f.A, 333 * b, axis=0))
        f.q = np.roll(f.q, 7 * b) * (1.0 + 0.25 * b)
        f.l, f.u = f.l * (1.0 + 0.1 * b), f.u * (1.0 + 0.1 * b)
        out.append(f)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# The reference: a direct solve of the reduced KKT system that never forms P
# ---------------------------------------------------------------------------------------------------------------------
def bound_vector(f, y):
    return np.where(y < 0, f.l, np.where(y > 0, f.u, 0.0))


def direct(f, y, delta=0.0):
    """x and the multipliers (full length m, 0 on inactive rows) of  [P + δI, A_act'; A_act, -δI] [x; λ] = [-q; bound]:  P + δI = D + U U' through
    Woodbury, λ from the Cholesky factor of the Schur complement  A_act (P + δI)^-1 A_act' + δI."""
    act = np.flatnonzero(y != 0)
    dt = f.d + delta
    Ud = f.U / dt[:, None]
    cap = f.U.T @ Ud
    cap[np.diag_indices_from(cap)] += 1.0
    c8 = sla.cho_factor(cap, lower=True)

    def pinv(R):
        T = R / (dt[:, None] if R.ndim == 2 else dt)
        return T - Ud @ sla.cho_solve(c8, f.U.T @ T)

    Aa = np.ascontiguousarray(f.A[act])
    PiAt = pinv(np.ascontiguousarray(Aa.T))
    S = Aa @ PiAt
    S[np.diag_indices_from(S)] += delta
    lam = sla.cho_solve(sla.cho_factor(S, lower=True, overwrite_a=True), -(PiAt.T @ f.q) - bound_vector(f, y)[act])
    x = pinv(-f.q - Aa.T @ lam)
    full = np.zeros(f.m)
    full[act] = lam
    return x, full


def dense_direct(P, q, A, l, u, y, delta=0.0):
    """np.linalg.solve on the dense reduced system (the small member, the tall case)."""
    n = P.shape[0]
    act = np.flatnonzero(y != 0)
    Aa = A[act]
    K = np.block([[P + delta * np.eye(n), Aa.T], [Aa, -delta * np.eye(act.size)]])
    t = np.linalg.solve(K, np.concatenate([-q, np.where(y[act] < 0, l[act], u[act])]))
    return t[:n], K


# ---------------------------------------------------------------------------------------------------------------------
# The refinement loop, restated over a product  (t, δ) -> K t + δ blkdiag(I, -mask) t
# bug: 0 none; 1 columns >= B ignored in the row dot; 2 columns >= B ignored in the column accumulation; 3 the mask ignored on inactive rows;
# 4 the δ term dropped from the multiplier block
# ---------------------------------------------------------------------------------------------------------------------
class StructuredK:
    """The masked KKT product over the family's d, U, A in the arithmetic of ``T`` (numpy.float64: the restatement; numpy.float32: the emulation).
    Only the active rows of A are touched (bug 3: all of them); inactive entries of the multiplier block stay exactly 0, as on the device."""

    def __init__(self, f, y, T=np.float64, bug=0):
        self.n, self.m, self.B, self.T, self.bug = f.n, f.m, f.B, T, bug
        self.rows = np.arange(f.m) if bug == 3 else np.flatnonzero(y != 0)
        self.A = np.ascontiguousarray(f.A[self.rows], dtype=T)
        self.d, self.U = f.d.astype(T), f.U.astype(T)

    def __call__(self, t, delta):
        n, T, B = self.n, self.T, self.B
        tx, w = t[:n], t[n:][self.rows]
        ax = self.A[:, :B] @ tx[:B] if self.bug == 1 else self.A @ tx
        at = self.A.T @ w
        if self.bug == 2:
            at[B:] = 0
        out = np.zeros(n + self.m, T)
        out[:n] = self.d * tx + self.U @ (self.U.T @ tx) + at + T(delta) * tx
        out[n + self.rows] = ax - T(0.0 if self.bug == 4 else delta) * w
        return out


class DenseK:
    """The same product over dense P and the active rows of A (the small member against the oracle, the tall case)."""

    def __init__(self, P, A, y, T=np.float64, bug=0):
        self.n, self.m, self.T, self.bug = P.shape[0], A.shape[0], T, bug
        self.rows = np.flatnonzero(y != 0)
        self.P, self.A = P.astype(T), np.ascontiguousarray(A[self.rows], dtype=T)

    def __call__(self, t, delta):
        n, T = self.n, self.T
        tx, w = t[:n], t[n:][self.rows]
        out = np.zeros(n + self.m, T)
        out[:n] = self.P @ tx + self.A.T @ w + T(delta) * tx
        out[n + self.rows] = self.A @ tx - T(0.0 if self.bug == 4 else delta) * w
        return out


def minres_t(matvec, b, tol, maxit, x0, T):
    """polish_oracle_np.minres statement by statement with every vector and every scalar in ``T`` (at numpy.float64 it returns the oracle's bits)."""
    x = np.array(x0, dtype=T)
    bnorm = T(np.sqrt(b @ b))
    if bnorm == 0:
        return np.zeros_like(x), 0, 0.0, 0
    r1 = b - matvec(x)
    y = r1.copy()
    beta1 = T(np.sqrt(r1 @ y))
    if not np.isfinite(beta1):
        return x, 1, math.nan, 0
    if beta1 <= T(tol) * bnorm:
        return x, 0, float(beta1 / bnorm), 0
    oldb, beta, dbar, epsln, phibar, cs, sn = T(0), beta1, T(0), T(0), beta1, T(-1), T(0)
    w = np.zeros_like(x); w2 = np.zeros_like(x); r2 = r1.copy()
    flag, itn = 1, 0
    tiny = T(np.finfo(np.float64).eps)
    for itn in range(1, maxit + 1):
        s = T(1) / beta
        v = s * y
        y = matvec(v)
        if itn >= 2:
            y = y - (beta / oldb) * r1
        alfa = T(v @ y)
        y = y - (alfa / beta) * r2
        r1 = r2
        r2 = y
        oldb = beta
        beta = T(np.sqrt(r2 @ y))
        oldeps = epsln
        delta = cs * dbar + sn * alfa
        gbar = sn * dbar - cs * alfa
        epsln = sn * beta
        dbar = -cs * beta
        gamma = max(T(np.sqrt(gbar * gbar + beta * beta)), tiny)
        cs = gbar / gamma
        sn = beta / gamma
        phi = cs * phibar
        phibar = sn * phibar
        w1 = w2
        w2 = w
        w = (v - oldeps * w1 - delta * w2) / gamma
        x = x + phi * w
        if not np.isfinite(phibar):
            break
        if phibar <= T(tol) * bnorm:
            flag = 0
            break
        if beta == 0:
            flag = 0
            break
    return x, flag, float(phibar / bnorm), itn


def refine(K, g, numItrPolish, δ, ϵMinres, numItrMinres):
    """SolveQuadraticProgram.m:307-325 over the product ``K`` (polish_oracle_np.Polish with the product factored out): fp64 through the oracle's
    minres, fp32 through its copy.  Returns (t, flag, per-call iteration counts); t is None when the last call did not converge."""
    T = K.T
    g = g.astype(T)
    t, tt, flag, counts = np.zeros(g.size, T), np.zeros(g.size, T), -1, []
    for _ in range(numItrPolish):
        rhs = g - K(t, 0.0)
        if T is np.float64:
            tt, flag, _, it = PO.minres(lambda v: K(v, δ), rhs, ϵMinres, numItrMinres, tt)
        else:
            tt, flag, _, it = minres_t(lambda v: K(v, δ), rhs, ϵMinres, numItrMinres, tt, T)
        counts.append(it)
        if flag:
            return None, flag, counts
        t = t + tt
    return t, flag, counts


def rhs_vector(f, y):
    return np.concatenate([-f.q, bound_vector(f, y)])


def run_params(case_or_dtype, run):
    dtype = case_or_dtype if isinstance(case_or_dtype, str) else case_or_dtype.dtype
    return dict((RUN_A if run == "A" else RUN_B)[dtype])


def restate(f, y, dtype, run, T=np.float64, bug=0, numItrMinres=100000):
    """x of the restated refinement loop (None when it ends with flag != 0), the flag and the per-call counts."""
    t, flag, counts = refine(StructuredK(f, y, T, bug), rhs_vector(f, y), numItrMinres=numItrMinres, **run_params(dtype, run))
    return (None if t is None else t[:f.n].astype(np.float64)), flag, counts


def budget(key):
    """numItrMinres of a device run: 4 x the largest per-call count of the restatement."""
    return 4 * ITS[key]


def bound(dtype, key, run):
    """The bound on |x - x_ref|_inf / max(1, |x_ref|_inf) of a run."""
    if dtype == "f64":
        return TOL64_A if run == "A" else 100.0 * DIST_B[key]
    return min(100.0 * EMU_F32[(key, run)], CAP32)
