"""The case table of tests/test_gpu_batch_bands.py (GPU) and tests/test_batch_bands_cpu.py (CPU guards): the lock-step batch of dense QPs
(BatchedDenseSolver::solve_batch, qps_dense_batch.hip; every launch carries blockIdx.y = QP) in every band of its count- and width-dependent launch
plans, both types, against the structured fp64 reference of tests/width_band_cases.py run on every QP of the batch.  Plain importable helper, no
device needed.  The handle reports ``sweepVariant`` and ``trsvBlock`` only (asserted per QP on the GPU); everything else is read off the dispatch
code, restated below and held against every case's claim by the CPU guards.

The dispatch code, restated (NP = roundup(n, 64), MP = roundup(m, 64), VN = 2 fp64 / 4 fp32):
  apass_plan         k_pass.hip:16-30.  total = 1024 workgroups when the problem is one column chunk wide (NP <= TH * VN, :23) and count > 1, else
                     256 (:24); target = 1 when count >= total, else total / count in integers (:25); rpw = ceil(MP / target) rounded up to a multiple
                     of 4 (:26-27); slabs per QP = ceil(MP / rpw) (:29); the last workgroup holds MP - (slabs - 1) * rpw rows.
  pass_route         k_pass.hip:13 and :43-53: width_band_cases.pass_route, unchanged by the count.
  admm_small_batch_supported   k_small.hip:527-530: NP in {64, 128}, MP >= 64 and MP / 64 <= 2 (fp64) / 4 (fp32) leaves the lock-step loop for the
                     one-workgroup-per-QP kernel (qps_dense_batch.hip:171, only while the sweep is one block).
  pick_nb            dense_chol.h:15-21: a request is rounded down to a power-of-two multiple of 64, then halved while half of it covers NP.
  chol_sweep_variant dense_chol.h:25-29: nb < NP -> 1 (one launch per block phase), else 2 when sweep_fused_supported (1024 <= NP), else 3.
  sweep_fused_slabs  k_trsv.hip:246-260.  Wave-per-row kernel (NP <= 64 * VN * 8, :229): min(256 / count, NP / 16), one slab when count >= 256
                     (:248-249); the instantiation is <KCW 4> up to 64 * VN * 4 and <KCW 8, single buffer> beyond (:282-283).  Chunked kernel:
                     kc = ceil(NP / (512 * VN)), total = 256 for one QP and 1024 / 512 / 256 for kc 1 / 2 / more in a batch (:256), slabs =
                     min(NP / RB, total / count) (:257-259) with RB = sweep_rb_for(kc) (:239-244).  DenseChol::sweeps (dense_chol.h:87) puts
                     slabs * NP into bw.vout and bx.mat as the stride between the slab sets of two QPs.
  refactor_changed   qps_dense_batch.hip:114: together = 2 * len(changed) >= count -> one batched re-factorisation, else the QPs of ``changed``
                     one by one (:122); with rebuild_slabs slab 0 of A'(rho z - y) is re-formed by a column GEMV and the others are cleared (:123-128).
  device bytes       the allocation list of the BatchedDenseSolver constructor (qps_dense_batch.hip:46-60) as ``device_bytes``.

The problem family.  width_band_cases.Family with a member index: QP b of a batch draws every array (d, U, A, q, l, u, x0) from its own stream
make_rng(2718, 2 + b) and multiplies A by its own scale 1.6 (1 + 0.5 frac(0.618... b)) (all different; 1.6 keeps a quarter of the rows of every shape but one at a bound -- the
200 x (150, 500) case, with more than three rows to a variable, also shrinks l and u to a fifth, ``tight``), so that a kernel that reads the matrix, a
slab set or a vector of another QP is far outside every bound (CPU guard: the reference of member b run on the matrices of member b' moves x by
at least 1000 x the bound, every ordered pair of every case; batches of more than 3 QPs run the pairs through a dense multi-column restatement
of the same loop, which is first held to the structured reference on the diagonal, and the cases of 200 and 1030 QPs run all K iterations on 25 partners of
every member and the first iteration on all the others, ``pair_columns``).  At least a quarter of the rows of every member sit
at a bound after the K iterations.  ``B`` as in the width bands: the first column of the top chunk the sweep instantiation uses (wave kernel:
64 * VN columns a chunk), or of the last 64-column block where no chunked sweep runs (NP = 192, 128); columns >= B carry WEIGHT.

Rows.  m = 300 would give rpw = 4 everywhere (one tile per workgroup, no ragged tail), so the wide cases keep the 2130 rows of the width bands:
MP = 2176, and the last real row (2129) falls inside a workgroup in every plan below.

Fixed-K cases (``CASES``): K = 20, a check every 10, eps = 0, rho = 0.1, sigma and alpha of the width bands, non-zero warm starts; every QP is
compared with admm_loop(Structured(member)) on x, z, y, resPrim, resDual.  Position independence: the three count = 3 fp64 cases at n = 150, 1000
and 1092 are solved a second time with the members in reverse order, and QP b must equal QP count - 1 - b of the other handle bit for bit.

Bug models of the CPU guards (``BugStructured``), each moving at least one compared quantity of every member it is run on by 100 x its bound:
  a   QP b takes the A of QP b + 1 in the row dot of the plain and the check pass;
  b   the rows of the last workgroup that holds a real row are left out of A'(rho z - y) (rho z - y is non-zero there: asserted);
  c   the entries of the right-hand side in the last NP / slabs range that holds a real entry are ignored by the solve (a lost sweep slab; for
      sweepVariant 1 the last diagonal block; not applicable to the two-GEMV sweep, which has no slabs);
  d   width_band_cases' bugs 1-3: columns >= B ignored in the row dot, in the column accumulation, by the solve.

Per-QP rho (``RHO_CASES``): R1 / R2 6 x (150, 170), R3 3 x (1000, 300), adptRho with fctrRho = 2 to eps = 1e-6, against c_oracle.solve per QP.  The
per-member scales on A were searched on the CPU (``rho_trace`` re-runs the oracle with numIterations stepped by the check period) so that R1 takes
the QP-by-QP branch of refactor_changed at its first switch, R2 the batched one and later a lone switch after another QP has stopped, R3 both.

Not covered: the 1024-thread pass in a batch (NP > 8192 fp64: two such QPs are 17 GB of device matrices, and the per-QP offsets are the same
template code as at 512 threads); count >= 256 at NP >= 1024; polishing in a batch (test_gpu_parity.py and test_gpu_polish_bands.py run it).

Bounds.  fp64: TOL["f64"] of loop_param_cases.py.  fp32: the rule of width_band_cases.bounds -- 100 x the error of the DenseF32 emulation against
the fp64 reference, recorded once per case and member in EMU_F32 (``PYTHONPATH=. python tests/batch_band_cases.py`` prints the table; the CPU guards repeat the
emulation for n <= 2052), never looser than TOL["f32"].

Measured on an MI355X (printed before every assertion, run with -s; largest figure over the QPs of a case against its bound; wall = the whole test,
members, references and handle included).  No case came near its bound except one fp32 residual, whose bound is 100 x a single small draw.
  fp64 fixed K   key: x / z / y / resPrim / resDual against 1e-9 / 1e-9 / 1e-8 / 1e-9 / 1e-9, wall
                 n150-c3        4.6e-14 / 2.0e-13 / 4.9e-14 / 2.5e-13 / 8.8e-13   0.2 s      n150-c200    1.4e-13 / 6.4e-13 / 6.5e-14 / 2.8e-13 / 9.2e-12   1.8 s
                 n120-c1030     8.4e-13 / 2.9e-12 / 4.6e-13 / 2.4e-12 / 2.1e-11   3.4 s      n150-c3-nb64 4.6e-14 / 2.0e-13 / 4.9e-14 / 2.5e-13 / 8.8e-13   0.0 s
                 n1000-c3       1.9e-13 / 9.1e-13 / 1.2e-13 / 3.9e-13 / 4.7e-12   0.5 s      n1000-c20    2.9e-13 / 9.5e-13 / 1.9e-13 / 7.8e-13 / 1.4e-11   3.9 s
                 n1000-c3-nb512 1.9e-13 / 9.1e-13 / 1.2e-13 / 3.9e-13 / 4.7e-12   0.6 s      n1092-c3     1.1e-13 / 5.0e-13 / 8.6e-14 / 2.0e-13 / 2.5e-12   0.6 s
                 n2052-c2       6.7e-15 / 4.4e-14 / 8.2e-15 / 1.1e-14 / 1.4e-12   0.5 s      n4100-c2     3.2e-15 / 2.8e-14 / 3.6e-15 / 1.3e-14 / 2.0e-13   0.7 s
                 (the wall of the 20-, 200- and 1030-QP cases is the CPU reference of every member: 3.7, 1.7 and 3.1 s; handle and solve 0.1 to 0.3 s)
  fp32 fixed K   key: the QP nearest its bound in x / z / y, measured against bound (100 x that member's emulation error), wall
                 n1000-c3  8.9e-7 / 3.9e-6 / 9.3e-7 against 7.7e-5 / 2.1e-4 / 3.4e-5   0.5 s      n1092-c3  7.6e-7 / 3.2e-6 / 8.2e-7 against 5.7e-5 / 1.2e-4 / 3.5e-5   0.6 s
                 n2040-c2  1.2e-6 / 3.1e-6 / 8.5e-7 against 8.4e-5 / 2.2e-4 / 5.0e-5   0.5 s      n2052-c2  4.7e-7 / 2.0e-6 / 6.3e-7 against 4.7e-5 / 1.7e-4 / 3.5e-5   0.6 s
                 n4100-c2  8.0e-7 / 2.2e-6 / 5.5e-7 against 6.6e-5 / 2.3e-4 / 4.3e-5   0.7 s      n150-c3   3.5e-7 / 8.6e-7 / 4.3e-7 against 4.9e-5 / 8.1e-5 / 2.4e-5   0.0 s
                 residuals: resPrim <= 8.0e-7 and resDual <= 1.9e-5, each at most about a fifth of its bound but resPrim of QP 2 of n150-c3: 3.7e-7 against 9.4e-7 (the
                 emulation's own draw there is 9.4e-9, forty times below the 3e-7 the device and the other members' emulations show).
  position       the three reversed batches equal the forward ones bit for bit in x, z, y and both residuals.
  per-QP rho     R1 / R2 / R3: flag, stopping iteration and numRefactor of every QP equal the oracle's; x within 2.6e-14 (absolute) against 1e-5, z 3.0e-14 and
                 y 2.1e-14 against 1e-9 / 1e-8 (frozen QPs included), residuals 2.1e-14 against 1e-9, rhoFinal 2.9e-12 against 1e-9; wall 0.0 / 0.0 / 0.3 s.
                 fp32 run of R1: equal flags, stopping iterations and refactor counts, x within 1.0e-6 against 5e-3."""
import copy
from collections import namedtuple

import numpy as np
import scipy.linalg as sla

import width_band_cases as W
from loop_param_cases import TOL

K, PERIOD, RHO, SIGMA, ALPHA = W.K, W.PERIOD, W.RHO, W.SIGMA, W.ALPHA
VN, SZ = W.VN, {"f64": 8, "f32": 4}
roundup = W.roundup
GC_RT = 32                                                             # k_loop.hip:93, rows per tile of the column GEMV
DEVICE_CAP, HOST_CAP = 3 * 2 ** 30, 2 ** 30


# ---------------------------------------------------------------------------------------------------------------------
# The dispatch code, restated (file and line in the docstring above)
# ---------------------------------------------------------------------------------------------------------------------
Plan = namedtuple("Plan", "total target rpw slabs last")


def apass_plan(dtype, NP, MP, count):
    vn = VN[dtype]
    if NP > 8 * 1024 * vn or MP <= 0:
        return None
    th = 1024 if NP > 8 * 512 * vn else 512
    total = 1024 if (NP <= th * vn and count > 1) else 256
    target = 1 if count >= total else total // max(count, 1)
    rpw = roundup(-(-MP // target), 4)
    slabs = -(-MP // rpw)
    return Plan(total, target, rpw, slabs, MP - (slabs - 1) * rpw)


pass_route = W.pass_route


def admm_small_batch_supported(dtype, NP, MP):
    return MP >= 64 and NP in (64, 128) and MP // 64 <= (2 if dtype == "f64" else 4)


def pick_nb(dtype, requested, NP):
    nb = requested if requested > 0 else (32768 if W.sweep_fused_supported(dtype, NP) else 4096)
    p = 64
    while p * 2 <= nb:
        p *= 2
    nb = p
    while nb > 64 and nb // 2 >= NP:
        nb //= 2
    return nb


def chol_sweep_variant(dtype, NP, nb):
    if nb < NP:
        return 1
    return 2 if W.sweep_fused_supported(dtype, NP) else 3


def sweep_fused_slabs(dtype, NP, count):
    """(kernel form, KC or KCW, RB, slabs per QP) of the fused sweep; RB is None for the wave kernel."""
    vn = VN[dtype]
    if NP <= 64 * vn * 8:
        per = 1 if count >= 256 else 256 // max(count, 1)
        return ("wave", 4 if NP <= 64 * vn * 4 else 8, None, max(1, min(per, NP // 16)))
    kc = -(-NP // (512 * vn))
    rb = 1 if NP > 8 * 512 * vn else W.sweep_rb_for(kc)
    total = 256 if count <= 1 else (1024 if kc <= 1 else 512 if kc == 2 else 256)
    per = 1 if count >= total else total // count
    KC = (12 if kc <= 12 else 16) if kc > 8 else (1 if kc <= 1 else 2 if kc <= 2 else 4 if kc <= 4 else 8)
    return ("fused", KC, rb, min(NP // rb, per))


def sweep_route(dtype, NP, nb, count):
    """("block", blocks) / ("gemv",) / ("wave", KCW, slabs) / ("fused", KC, RB, slabs): what DenseChol::sweeps launches."""
    v = chol_sweep_variant(dtype, NP, nb)
    if v == 1:
        return ("block", -(-NP // nb))
    if v == 3:
        return ("gemv",)
    form, kc, rb, slabs = sweep_fused_slabs(dtype, NP, count)
    return (form, kc, slabs) if form == "wave" else (form, kc, rb, slabs)


def refactor_together(changed, count):
    return 2 * len(changed) >= count


def device_bytes(dtype, n, m, count):
    """The allocation list of the BatchedDenseSolver constructor (qps_dense_batch.hip:46-60)."""
    NP, MP, s, c = roundup(n, 64), roundup(m, 64), SZ[dtype], count
    nn, slabs, tiles = NP * NP, apass_plan(dtype, NP, MP, count).slabs, -(-MP // GC_RT)
    elems = c * MP * NP + 6 * c * nn + c * (NP // 64) * 4096 + 9 * c * NP + 4 * c * MP             # A; P PI AA M S tmp; dinv; q x xp xres xx tt yv Px Aty; l u z y
    elems += max(c * slabs, apass_plan(dtype, NP, MP, 1).slabs, tiles, 1) * NP + c * slabs * NP + max(tiles, 1) * NP   # part, part2, part_tmp
    elems += c * max(sweep_fused_slabs(dtype, NP, count)[3], 1) * NP                                # sw_part
    small = 2 * 4 * (count + 4) + 2 * 8 * (count + 4) + 8 * 16 * c + 8 * 8 * c                    # fail d_active; d_rho d_rhorho; scratch; res_dev
    return s * elems + small + 8 * (max(MP * NP, nn) + 64)                                         # + the fp64 staging buffer


def host_bytes(n, m, count):
    return 8 * count * (n * n + m * n + 2 * n + 2 * m)                 # P, A, q, x0, l, u in fp64


# ---------------------------------------------------------------------------------------------------------------------
# The fixed-K cases
# ---------------------------------------------------------------------------------------------------------------------
# trsv: the trsvBlock request (0: default); pass_: (TH, KC, R plain, R check); plan: Plan; sweep: sweep_route; variant / nb: what the handle reports
BCase = namedtuple("BCase", "key dtype n m count trsv NP MP B pass_ plan sweep variant nb tight", defaults=(1.0,))
M = W.M_ROWS
CASES = [
    BCase("f64-n150-c3", "f64", 150, 170, 3, 0, 192, 192, 128, (512, 1, 4, 4), Plan(1024, 341, 4, 48, 4), ("gemv",), 3, 256),          # minimum rpw; 1024 / 3 not an integer
    BCase("f64-n150-c200", "f64", 150, 500, 200, 0, 192, 512, 128, (512, 1, 4, 4), Plan(1024, 5, 104, 5, 96), ("gemv",), 3, 256, 0.2),   # many QPs, few fat slabs, ragged last
    BCase("f64-n120-c1030", "f64", 120, 270, 1030, 0, 128, 320, 64, (512, 1, 4, 4), Plan(1024, 1, 320, 1, 320), ("gemv",), 3, 128),      # count >= total: one slab per QP
    BCase("f64-n150-c3-nb64", "f64", 150, 170, 3, 64, 192, 192, 128, (512, 1, 4, 4), Plan(1024, 341, 4, 48, 4), ("block", 3), 1, 64),  # batched variant 1
    BCase("f64-n1000-c3", "f64", 1000, M, 3, 0, 1024, 2176, 896, (512, 1, 4, 4), Plan(1024, 341, 8, 272, 8), ("wave", 8, 64), 2, 1024),   # the C4 kernel in fp64; NP / 16 limit
    BCase("f64-n1000-c20", "f64", 1000, M, 20, 0, 1024, 2176, 896, (512, 1, 4, 4), Plan(1024, 51, 44, 50, 20), ("wave", 8, 12), 2, 1024),  # 256 / count limit
    BCase("f64-n1000-c3-nb512", "f64", 1000, M, 3, 512, 1024, 2176, 896, (512, 1, 4, 4), Plan(1024, 341, 8, 272, 8), ("block", 2), 1, 512),
    BCase("f64-n1092-c3", "f64", 1092, M, 3, 0, 1152, 2176, 1024, (512, 2, 4, 4), Plan(256, 85, 28, 78, 20), ("fused", 2, 2, 170), 2, 2048),   # first NP past the wave kernel
    BCase("f64-n2052-c2", "f64", 2052, M, 2, 0, 2112, 2176, 2048, (512, 4, 4, 2), Plan(256, 128, 20, 109, 16), ("fused", 4, 4, 128), 2, 4096),
    BCase("f64-n4100-c2", "f64", 4100, M, 2, 0, 4160, 2176, 4096, (512, 8, 2, 1), Plan(256, 128, 20, 109, 16), ("fused", 8, 1, 128), 2, 8192),
    BCase("f32-n1000-c3", "f32", 1000, M, 3, 0, 1024, 2176, 768, (512, 1, 4, 4), Plan(1024, 341, 8, 272, 8), ("wave", 4, 64), 2, 1024),    # the only NP that reaches KCW 4
    BCase("f32-n1092-c3", "f32", 1092, M, 3, 0, 1152, 2176, 1024, (512, 1, 4, 4), Plan(1024, 341, 8, 272, 8), ("wave", 8, 72), 2, 2048),   # entry of KCW 8 in fp32
    BCase("f32-n2040-c2", "f32", 2040, M, 2, 0, 2048, 2176, 1792, (512, 1, 4, 4), Plan(1024, 512, 8, 272, 8), ("wave", 8, 128), 2, 2048),  # last wave NP, top chunk live
    BCase("f32-n2052-c2", "f32", 2052, M, 2, 0, 2112, 2176, 2048, (512, 2, 4, 4), Plan(256, 128, 20, 109, 16), ("fused", 2, 2, 256), 2, 4096),
    BCase("f32-n4100-c2", "f32", 4100, M, 2, 0, 4160, 2176, 4096, (512, 4, 4, 2), Plan(256, 128, 20, 109, 16), ("fused", 4, 4, 128), 2, 8192),
    BCase("f32-n150-c3", "f32", 150, 170, 3, 0, 192, 192, 128, (512, 1, 4, 4), Plan(1024, 341, 4, 48, 4), ("gemv",), 3, 256),
]
BY_KEY = {c.key: c for c in CASES}
POSITION_KEYS = ("f64-n150-c3", "f64-n1000-c3", "f64-n1092-c3")
PAIRWISE_DIRECT = 3                                                    # up to this count the pair guard runs the structured reference itself
PAIRWISE_FULL = 20                                                     # up to this count every ordered pair runs all K iterations (``pair_columns``)
EMU_MAX_N = 2052                                                       # the CPU guards repeat the fp32 emulation up to this n


def case_id(c):
    return c.key


def member_scale(b):
    return 1.6 * (1.0 + 0.5 * ((b * 0.6180339887498949) % 1.0))


_members = {}


def members(case):
    """The Family members of a case, cached (one case at a time); treat as read-only."""
    key = (case.n, case.m, case.count, case.B)
    if key not in _members:
        _members.clear()
        _members[key] = [W.Family(case.n, case.B, m=case.m, member=b, scale=member_scale(b), tight=case.tight) for b in range(case.count)]
    return _members[key]


def crossed(fb, fm):
    """The vectors (q, l, u, x0) of member ``fb`` on the matrices (d, U, A) of member ``fm``; shares fm's factor cache."""
    g = copy.copy(fm)
    g.q, g.l, g.u, g.x0 = fb.q, fb.l, fb.u, fb.x0
    return g


def reference(f):
    return W.admm_loop(W.Structured(f))


def dense_ops(fm):
    """(A, M^-1) of a member, M = P + sigma I + rho A'A formed densely: the explicit inverse turns the loop below into GEMMs; the guard that uses
    it first holds its result to the structured reference."""
    A = fm.A
    Mx = fm.U @ fm.U.T + RHO * (A.T @ A)
    Mx[np.diag_indices_from(Mx)] += fm.d + SIGMA
    return A, sla.cho_solve(sla.cho_factor(Mx, lower=True, overwrite_a=True), np.eye(fm.n))


def dense_multi_loop(ops, Q, L, U, X0, iterations=K):
    """admm_loop (SolveQuadraticProgram.jl:45-61, fixed rho, eps = 0) for many QPs at once on the matrices behind ``ops``: column j runs
    (Q[:, j], L[:, j], U[:, j], X0[:, j]).  Returns x of every column.  The pair guard of the cases of more than PAIRWISE_DIRECT QPs runs on it."""
    A, Mi = ops
    X, Z, Y = X0.copy(), np.zeros_like(L), np.zeros_like(L)
    for _ in range(iterations):
        XX = Mi @ (SIGMA * X - Q + A.T @ (RHO * Z - Y))
        ZZ = A @ XX
        X = ALPHA * XX + (1 - ALPHA) * X
        V = ALPHA * ZZ + (1 - ALPHA) * Z
        Z = np.clip(V + Y / RHO, L, U)
        Y = Y + RHO * (V - Z)
    return X


def first_x(ops, Q, X0):
    """x of every column after the first iteration (z = y = 0 there: no product with A)."""
    return ALPHA * (ops[1] @ (SIGMA * X0 - Q)) + (1 - ALPHA) * X0


def pair_columns(count, o):
    """The members whose vectors run all K iterations on the matrices of member ``o`` in the pair guard: everyone up to PAIRWISE_FULL QPs; beyond
    that the 8 neighbours on either side (what a wrong per-QP stride reads) and 8 members spread over the batch -- every other ordered pair is
    held to the same factor after the first iteration only (4 x 10^4 and 10^6 full runs would take one and two minutes of CPU)."""
    if count <= PAIRWISE_FULL:
        return np.arange(count)
    near = (o + np.arange(-8, 9)) % count
    return np.unique(np.concatenate([near, (o + (np.arange(1, 9) * count) // 9) % count]))


# ---------------------------------------------------------------------------------------------------------------------
# Bug models
# ---------------------------------------------------------------------------------------------------------------------
def last_real_rows(case):
    """Rows of the last workgroup of the pass that holds a real row."""
    r0 = (case.m - 1) // case.plan.rpw * case.plan.rpw
    return r0, case.m


def last_sweep_range(case):
    """Entries of the right-hand side that the last sweep slab (variant 1: block) with a real entry stands for, or None (two-GEMV sweep)."""
    if case.sweep[0] == "gemv":
        return None
    w = case.nb if case.sweep[0] == "block" else max(1, case.NP // case.sweep[-1])
    return (case.n - 1) // w * w, case.n


class BugStructured(W.Structured):
    """Structured with the batch bug models: "a" (``other``: the member whose A the row dot reads), "b" (rows), "c" (entries)."""

    def __init__(self, f, model, case, other=None):
        super().__init__(f, 0)
        self.model, self.case, self.other = model, case, other

    def Ax(self, x, rows=slice(None), check=False):
        return self.other.A[rows] @ x if self.model == "a" else super().Ax(x, rows, check)

    def Atw(self, w, rows=slice(None), check=False):
        if self.model == "b" and not check:
            w = w.copy(); r0, r1 = last_real_rows(self.case); w[r0:r1] = 0.0
        return super().Atw(w, rows, check)

    def solve(self, r):
        if self.model == "c":
            r = r.copy(); e0, e1 = last_sweep_range(self.case); r[e0:e1] = 0.0
        return super().solve(r)


# ---------------------------------------------------------------------------------------------------------------------
# Bounds
# ---------------------------------------------------------------------------------------------------------------------
# Error of the fp32 emulation against the fp64 reference, per case and member (``PYTHONPATH=. python tests/batch_band_cases.py`` on the CPU).
EMU_F32 = {
    ("f32-n1000-c3", 0): dict(x=5.89e-07, z=2.05e-06, y=3.69e-07, resPrim=4.24e-07, resDual=6.45e-07),
    ("f32-n1000-c3", 1): dict(x=7.69e-07, z=2.09e-06, y=4.58e-07, resPrim=2.88e-07, resDual=7.81e-06),
    ("f32-n1000-c3", 2): dict(x=6.80e-07, z=1.60e-06, y=3.40e-07, resPrim=1.92e-07, resDual=3.97e-06),
    ("f32-n1092-c3", 0): dict(x=6.22e-07, z=1.24e-06, y=2.68e-07, resPrim=2.24e-07, resDual=4.04e-06),
    ("f32-n1092-c3", 1): dict(x=5.67e-07, z=1.88e-06, y=3.50e-07, resPrim=1.93e-08, resDual=6.73e-06),
    ("f32-n1092-c3", 2): dict(x=5.50e-07, z=2.30e-06, y=3.13e-07, resPrim=7.29e-07, resDual=1.05e-05),
    ("f32-n2040-c2", 0): dict(x=6.68e-07, z=2.25e-06, y=4.55e-07, resPrim=1.38e-06, resDual=2.15e-06),
    ("f32-n2040-c2", 1): dict(x=8.42e-07, z=2.38e-06, y=5.00e-07, resPrim=1.61e-07, resDual=5.79e-06),
    ("f32-n2052-c2", 0): dict(x=4.72e-07, z=1.75e-06, y=3.32e-07, resPrim=1.02e-06, resDual=9.19e-07),
    ("f32-n2052-c2", 1): dict(x=8.26e-07, z=1.61e-06, y=3.52e-07, resPrim=5.18e-07, resDual=1.06e-05),
    ("f32-n4100-c2", 0): dict(x=6.83e-07, z=2.29e-06, y=3.89e-07, resPrim=3.87e-07, resDual=9.75e-06),
    ("f32-n4100-c2", 1): dict(x=6.62e-07, z=2.75e-06, y=4.29e-07, resPrim=9.21e-08, resDual=6.95e-06),
    ("f32-n150-c3", 0): dict(x=4.61e-07, z=6.32e-07, y=2.68e-07, resPrim=1.54e-07, resDual=9.29e-07),
    ("f32-n150-c3", 1): dict(x=5.96e-07, z=8.07e-07, y=2.39e-07, resPrim=8.90e-07, resDual=9.83e-06),
    ("f32-n150-c3", 2): dict(x=4.92e-07, z=8.95e-07, y=2.65e-07, resPrim=9.37e-09, resDual=8.51e-06),
}


def emulation_error(case, b):
    f = members(case)[b]
    return W.errors(W.admm_loop(W.DenseF32(f)), reference(f), W.ADMM_KEYS)


def bounds(case, b):
    """The bound of every compared quantity of QP ``b`` of a case."""
    if case.dtype == "f64":
        return dict(TOL["f64"])
    emu, cap = EMU_F32[(case.key, b)], TOL["f32"]
    return {k: min(100.0 * emu[k], cap[k]) for k in cap}


# ---------------------------------------------------------------------------------------------------------------------
# Per-QP rho: the two branches of refactor_changed, frozen QPs
# ---------------------------------------------------------------------------------------------------------------------
# switches: ((check, QPs that switch at the top of the next iteration), ...); stops: the check every QP stops at -- what the CPU guard derives from the oracle
RhoCase = namedtuple("RhoCase", "key n m B scales switches stops")
RHO_PARAMS = dict(numIterations=600, numItrConv=PERIOD, epsAbs=1e-6, epsRel=1e-6, rho=RHO, sigma=SIGMA, alpha=ALPHA, adptRho=True, fctrRho=2.0)
RHO_PARAMS_F32 = dict(RHO_PARAMS, epsAbs=1e-4, epsRel=1e-4)
ABS_DEV_THR = 1e-5                                                     # RunTests.jl:58
MARGIN = 0.02                                                          # no decision within 2 % of its threshold (as the infeasibility and equilibration guards)
RHO_CASES = [
    RhoCase("R1-one-by-one", 150, 170, 128, (1.513, 0.456, 1.513, 0.456, 2.758, 1.513), ((20, (0, 2)), (60, (3,)), (70, (5,)), (80, (1,))), (60, 160, 70, 170, 90, 120)),
    RhoCase("R2-together", 150, 170, 128, (1.513, 1.513, 1.513, 1.121, 0.83, 1.513), ((20, (0, 1, 2, 3, 4)), (70, (5,))), (60, 90, 70, 80, 90, 120)),
    RhoCase("R3-wave-sweep", 1000, 300, 896, (0.83, 1.121, 0.338), ((20, (1, 2)), (60, (0,))), (90, 60, 100)),
]
RHO_BY_KEY = {c.key: c for c in RHO_CASES}


def rho_members(rc):
    return [W.Family(rc.n, rc.B, m=rc.m, member=b, scale=s) for b, s in enumerate(rc.scales)]


def oracle_solve(co, f, **params):
    x, io = co.solve(f.dense_P(), f.q, f.A, f.l, f.u, vX=f.x0, **params)
    io["x"] = x
    return io


def rho_trace(co, f, params=None):
    """The per-check record of one QP: c_oracle.solve re-run with numIterations stepped by the check period (the oracle keeps no record of its own).
    Entry k - 1 is the state after check k: the rho in force, the proposal, the residuals and their scales, the flag, x, z, y.  Ends with the check
    at which the QP stops."""
    params = dict(RHO_PARAMS if params is None else params)
    out, k = [], 0
    while True:
        k += 1
        it = k * params["numItrConv"]
        io = oracle_solve(co, f, **dict(params, numIterations=it))
        out.append(io)
        if io["convFlag"] != 1 or io["iterations"] < it or it >= params["numIterations"]:
            return out


def decisions(trace, params=None):
    """Per check: (switches at the top of the next iteration, stops, the quotients value / threshold of every decision taken at this check)."""
    params = RHO_PARAMS if params is None else params
    fctr, out = params["fctrRho"], []
    for io in trace:
        ratio = io["rhoProposed"] / io["rhoFinal"]
        qp, qd = io["resPrim"] / (params["epsAbs"] + params["epsRel"] * io["maxNormPrim"]), io["resDual"] / (params["epsAbs"] + params["epsRel"] * io["maxNormDual"])
        stops = io["convFlag"] != 1
        switches = (not stops) and io["iterations"] < params["numIterations"] and (ratio * fctr < 1 or ratio > fctr)
        out.append(dict(it=io["iterations"], switches=switches, stops=stops, flag=io["convFlag"], quotients=(ratio * fctr, ratio / fctr, max(qp, qd) if not stops else None, qp, qd)))
    return out


def margins_ok(dec):
    """No switching decision and no stopping decision within MARGIN of its threshold.  (A stop by convPrimDual needs both quotients below 1; going
    on needs the larger one above.)"""
    for d in dec:
        lo, hi, go, qp, qd = d["quotients"]
        if abs(lo - 1) < MARGIN or abs(hi - 1) < MARGIN:
            return False
        if d["stops"]:
            if d["flag"] != 3 or max(qp, qd) > 1 - MARGIN:
                return False
        elif go < 1 + MARGIN:
            return False
    return True


if __name__ == "__main__":
    for c in CASES:
        if c.dtype == "f32":
            for b in range(c.count):
                e = emulation_error(c, b)
                print(f'    ("{c.key}", {b}): dict(' + ", ".join(f"{k}={v:.2e}" for k, v in e.items()) + "),", flush=True)
