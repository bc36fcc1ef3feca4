"""The case table of tests/test_gpu_setup_bands.py (GPU) and tests/test_setup_bands_cpu.py (CPU guards): the setup chain of the dense solvers -- A'A on the
MFMA pipe, M = P + σI + ρA'A, the Cholesky chain, the explicit inverse by recursive doubling and the premultiplied form (k_setup.hip, driven by DenseChol in
dense_chol.h) -- in every band of the padded order NP = roundup(n, 64), both types, on systems whose exact solution is known.  Plain importable helper, no
device needed.

The systems (``problem``).  W symmetric with zero diagonal and off-diagonal entries from {-1, 0, 1}; P = W + d I with d = ceil(4 sqrt(n)) (the spectrum of W
lies within about +-2 sqrt(n): P is SPD, kappa(M) = 3 ... 12, and every 64 x 64 tile of P is dense); A m x n from {-1, 0, 1}; σ = 1, ρ = 0.5, so that
M = P + σI + ρA'A consists of half-integers; x* non-zero integers in [-3, 3] (+-3 on the real rows of the last block); q = -M x* (|q| < 2^24: exact in fp32 too).  With x = z = y = 0 the right-hand
side of the plugin pair, σx - q + A'(ρz - y) (LinearSystemSolvers.jl:134-136), is exactly M x*: the exact x~ is x*, the exact z~ is A x*.  On the device
A'A, PI and M are exact in both types; every error comes from the factor, the inverse and the sweeps.  ρ switch: linsys_solve(ρ2 = 2, changedΡ) with
x = (ρ2 - ρ1) A'A x* (integers times 1.5) and z = y = 0 has the right-hand side M2 x* exactly, on the refactor path that reuses the cached A'A.

The bands, restated from the dispatch code (``branches(n, m, dtype, ...)`` returns the set a handle reaches; the CPU guards assert that the table reaches both
sides of every threshold):
  chol_scratch_fits     qps_kernels.h:246-247; dense_chol.h:61 passes the scratch only when it fits, k_setup.hip:1008 takes the fused 128-column chain
                        with it and :1045-1054 the 64-column chain (k_potrf64 / k_trsm_panel / k_update_potrf / k_inv64) without: NP = 64 only.
  chol_steps            k_setup.hip:1012-1025: one step per two block columns while rows remain; g = rows below / 64, nt = g (g + 1) / 2 - 1,
                        avoid = batch == 1 and nt >= 256 and (fp32 or nt <= 1500) (:1020), ids = chol_update_ids(g, avoid) (tile_order.h:39).  nblk = 2 runs
                        no step, nblk = 3 one step with g = 1 and ids = 1 (the diagonal workgroup alone); an odd nblk leaves a 64-column tail block
                        (k_chol_update_diag: two = nblk - cbn >= 2, :754).
  gemm_plan             k_setup.hip:968-977: mirror-tile pairing of a triangular-operand product when ni nj batch >= 512 and the paired axis is even (:970);
                        the lower tiles of A'A on the 1-D XCD-aware order when ni (ni + 1) / 2 batch >= 512 (:974), lower_tile_ids rounds up to 8
                        (tile_order.h:20).
  sweep_gemms           k_setup.hip:1063-1100: per doubling level s < nb the nfull full pairs (batched over blockIdx.z when batch == 1, :1067-1070, looped
                        on the host otherwise, :1072-1076) and the ragged pair (:1080-1085); the premultiplied form (:1087-1100).
  pick_nb / premul      dense_chol.h:15-21 with sweep_fused_supported (k_trsv.hip:233); trsv_blocked_supported (k_trsv_blocked.hip:287-296) on a device that
                        holds the 256 workgroups co-resident: nb = 256 VN or 512 VN with at least two blocks.

Cases: ``SINGLE`` (stand-alone handles through linsys_init / linsys_solve; ``TRSV`` re-initialises n = 1600 and 3136 with other block sizes; ``RHO_SWITCH``),
``BATCH`` (QuadraticProgramBatch, one iteration at α = 1 from a zero start: the returned x is x~), ``BREAKDOWN`` (one diagonal entry of P set to -d: the
leading c x c block stays SPD, so the first non-positive pivot is column c exactly, reported 1-based by PotrfCol as QPS_ERR_FACTORIZATION).
Not covered: ProxQP, the shared-matrix batches (the ρ-scale SYRK on diag(sqrt(s)) A included) and the dense tail of the sparse L D L', which run the same
DenseChol with their own right-hand sides; fp32 orders beyond 4096; the QPS_CHOL_* / QPS_GEMM_* switches (test_tuning_knobs_do_not_change_results).

Bounds.  BOUND[dtype] = 8 x max(e_alg, e_ref, u) over all cases: e_alg the error max|x - x*| / max|x*| of ``restated_solve`` (numpy in that type: LAPACK
Cholesky, explicit inverse S of the factor, x = S'(S r) -- the device's algorithm), e_ref that of a LAPACK Cholesky solve, u the unit roundoff.  The factor
8 pays for the MFMA accumulation order and the Newton reciprocals that replace divisions; nothing comes from GPU output.  The largest figures are recorded
in E_MAX (the CPU guards recompute them for n <= 2112 and for n = 4096); they come from the ρ switch to ρ2 = 2: BOUND = 9.5e-14 (fp64), 4.6e-5 (fp32).
max|zz - A x*| is held to BOUND max|x*| max_i sum_j |A_ij| + NP u max|A x*|.

Measured on an MI355X (printed before every assertion, run with -s; "a against b" = largest figure of the cases against its bound).  No defect was found
and no case came near its bound: the device stays within 3 x the error of the numpy restatement.
  plugin pair fp64   x <= 2.5e-15 at ρ = 0.5 in all 15 orders (n = 40: 5.9e-16; n = 4096: 2.5e-15) and all re-initialised block sizes (n = 1600 and 3136,
                     trsvBlock 64 / 256 / 512 / 1024: <= 2.8e-15); after the switch to ρ2 = 2: 1.6e-15 / 4.3e-15 / 5.2e-15 (n = 130 / 1600 / 2112), back at ρ the
                     first figure to the last digit.  All against 9.5e-14.  z <= 1.1e-13 against 9.3e-12 ... 9.4e-10.
  plugin pair fp32   x 3.2e-7 (n = 40) ... 1.6e-6 (n = 4096); block sizes 64 / 256 / 1024 / 2048: <= 1.2e-6; ρ2: 8.0e-7 / 2.9e-6 / 2.4e-6.  All against 4.6e-5.
                     z <= 9.2e-5 against 4.5e-3 ... 4.6e-1.
  batch              fp64 x <= 7.4e-16 (130 x 3), 2.4e-15 (576 x 12), 2.1e-15 (640 x 10); fp32 5.6e-7, 1.3e-6, 1.1e-6; iterations == 1 for every QP.
  breakdown          QPS_ERR_FACTORIZATION with "non-positive pivot at column c + 1" at all eight positions in both types, "QP 1 of the batch" for the batch.
  wall               52 tests in 4.7 s; n = 4096 fp64 2.5 s (the host matrix), everything else <= 0.3 s.
Three deliberate breaks of k_setup.hip were run on the hardware, none touching an address, and failed exactly the cases ``branches`` sends through the
broken line: the mirror tile of a ktri 2 pair skipped (n = 3072, 4096 and n = 3136 at trsvBlock 1024 only -- the premultiplied form; x off by 18 ... 3e5);
the last tile of an avoided update launch skipped (n = 1600 and every larger order, not 1536; 9e-2 ... 2e-1); the last tile of the 1-D order of A'A skipped
(n >= 2048 and the batches 576 x 12 and 640 x 10, not 1984 or 130 x 3; 3e-1 ... 1.2).  The same figures in both types."""
import math
from collections import namedtuple

import numpy as np
import scipy.linalg as sla

from quadraticprogramsolver_amd.generator import make_rng

SIGMA, RHO, RHO2 = 1.0, 0.5, 2.0
DTYPES = ("f64", "f32")
NPDT = {"f64": np.float64, "f32": np.float32}
U = {"f64": 2.0 ** -53, "f32": 2.0 ** -24}
VN = {"f64": 2, "f32": 4}
SEED = 3141

# Largest error of the restated algorithm / of the LAPACK solve over all cases (``cpu_errors``), measured on the CPU: fp64 4.9e-15 / 8.5e-15, fp32
# 2.7e-6 / 4.1e-6 (all four at ρ2 = 2, n = 1600 and 2112).  Each is a single draw of a rounding error that moves with the blocking of the BLAS at hand, so the
# record is 1.4 x the measured figure: the CPU guard, which wants 8 x the recomputed maximum <= BOUND <= 16 x it, then accepts 0.7 ... 1.4 x the measurement.
E_MAX = {"f64": dict(alg=1.4 * 4.9e-15, ref=1.4 * 8.5e-15), "f32": dict(alg=1.4 * 2.7e-6, ref=1.4 * 4.1e-6)}
BOUND = {dt: 8.0 * max(E_MAX[dt]["alg"], E_MAX[dt]["ref"], U[dt]) for dt in DTYPES}                   # fp64 9.5e-14, fp32 4.6e-5

Single = namedtuple("Single", "n m why")
SINGLE = [
    Single(40, 3, "NP 64: the scratch does not fit -> 64-column chain + k_inv64, no doubling level; padded rows of A and M"),
    Single(65, 65, "NP 128, nblk 2: one real row in block 2 and 63 identity rows; fused chain without a loop step; MP 128"),
    Single(130, 64, "nblk 3: odd tail block; one update launch with g = 1; ragged pair s = 128, s2 = 64"),
    Single(256, 64, "nblk 4: g = 2"),
    Single(320, 64, "nblk 5: g = 3 -> 1; ragged at s = 256"),
    Single(448, 130, "nblk 7: odd; K depth 192"),
    Single(1536, 64, "nblk 24: avoid never"),
    Single(1600, 64, "nblk 25: avoid in the first step only, odd"),
    Single(1664, 64, "nblk 26: avoid in the first step only, even"),
    Single(1984, 64, "nblk 31: A'A on the plain 2-D grid"),
    Single(2048, 64, "nblk 32: A'A in the 1-D order, 528 ids, no padding"),
    Single(2112, 64, "nblk 33: A'A in the 1-D order, 568 ids, 7 padding ids"),
    Single(3072, 64, "nblk 48: ragged pair at s = 2048 with s2 / 64 = 16: both products paired"),
    Single(3136, 64, "nblk 49: ragged pair at s = 2048 with s2 / 64 = 17: ktri 1 paired, ktri 2 not"),
    Single(4096, 64, "nblk 64: full pairs over blockIdx.z with pairing; fp64 first steps unavoided (nt > 1500), fp32 avoided throughout"),
]
TRSV = {1600: {"f64": (64, 256, 512, 1024), "f32": (64, 256, 1024, 2048)}, 3136: {"f64": (64, 256, 512, 1024), "f32": (64, 256, 1024, 2048)}}
RHO_SWITCH = (130, 1600, 2112)
Batch = namedtuple("Batch", "n m count why")
BATCH = [
    Batch(130, 64, 3, "6 x 3 tiles: 2-D grid; doubling looped on the host"),
    Batch(576, 64, 12, "45 x 12 >= 512: 1-D order inside a batch, 48 ids with 3 padding; odd nblk"),
    Batch(640, 64, 10, "55 x 10 >= 512: 56 ids"),
]
Breakdown = namedtuple("Breakdown", "n m count qp c why")
BREAKDOWN = [
    Breakdown(200, 64, 1, 0, 0, "first launch, first column"),
    Breakdown(200, 64, 1, 0, 63, "first launch, last column of L00"),
    Breakdown(200, 64, 1, 0, 64, "second block of a 128-column step"),
    Breakdown(200, 64, 1, 0, 127, "last column of the first step"),
    Breakdown(200, 64, 1, 0, 128, "first column factorised inside k_chol_update_diag"),
    Breakdown(200, 64, 1, 0, 199, "last real column"),
    Breakdown(40, 3, 1, 0, 39, "64-column chain"),
    Breakdown(130, 64, 3, 1, 70, "QP 1 of a batch"),
]


def single_id(c):
    return f"n{c.n}"


def batch_id(c):
    return f"n{c.n}x{c.count}"


def breakdown_id(c):
    return f"n{c.n}" + (f"x{c.count}-qp{c.qp}" if c.count > 1 else "") + f"-c{c.c}"


# ---------------------------------------------------------------------------------------------------------------------
# The systems
# ---------------------------------------------------------------------------------------------------------------------
class Problem:
    """P, A (Fortran order, float64 holding small integers), q = -M x*, xs = x*, AA = A'A, d; l, u = -/+ 1 (they do not enter x~)."""

    def __init__(self, n, m, stream):
        rng = make_rng(SEED, stream)
        self.n, self.m, self.d = n, m, float(math.ceil(4.0 * math.sqrt(n)))
        W = np.tril(rng.integers(-1, 2, size=(n, n)), -1).astype(np.float64)
        P = W + W.T
        P[np.diag_indices(n)] = self.d
        self.P = np.asfortranarray(P)
        self.A = np.asfortranarray(rng.integers(-1, 2, size=(m, n)).astype(np.float64))
        self.xs = rng.choice(np.array([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0]), size=n)
        tail = slice((n - 1) // 64 * 64, n)                              # the real rows of the last, ragged block: |x*| = 3, as visible as they can be
        self.xs[tail] = 3.0 * np.sign(self.xs[tail])
        self.AA = self.A.T @ self.A                                      # integers: exact
        self.q = -self.M(RHO) @ self.xs
        self.l, self.u = -np.ones(m), np.ones(m)

    def M(self, rho):
        M = self.P + rho * self.AA
        M[np.diag_indices(self.n)] += SIGMA
        return M

    def x_for_rho(self, rho):
        """The x of linsys_solve that makes the right-hand side σx - q equal to M(rho) x* exactly (σ = 1)."""
        return (rho - RHO) * (self.AA @ self.xs)

    def zbound(self, dtype):
        return BOUND[dtype] * np.abs(self.xs).max() * np.abs(self.A).sum(axis=1).max() + roundup(self.n, 64) * U[dtype] * np.abs(self.A @ self.xs).max()


_problems = {}


def problem(n, m, stream=0):
    """Cached; treat as read-only.  Small ones stay, of the large ones only the last (n = 4096 holds 0.4 GB)."""
    key = (n, m, stream)
    if key not in _problems:
        for k in [k for k in _problems if k[0] > 700]:
            del _problems[k]
        _problems[key] = Problem(n, m, stream)
    return _problems[key]


def batch_problems(c):
    return [problem(c.n, c.m, 1 + b) for b in range(c.count)]


def breakdown_problem(c):
    """(problems, the broken one): P[c, c] = -d in QP ``qp``; a fresh copy, the cached problem stays as it is."""
    base = batch_problems(c) if c.count > 1 else [problem(c.n, c.m)]
    P = base[c.qp].P.copy(order="F")
    P[c.c, c.c] = -base[c.qp].d
    return base, P


# ---------------------------------------------------------------------------------------------------------------------
# The algorithm, restated: padded M as k_make_PI / k_assemble_M build it, Cholesky, explicit inverse, two products
# ---------------------------------------------------------------------------------------------------------------------
def roundup(a, b):
    return (a + b - 1) // b * b


def padded(pr, rho=RHO, AA=None):
    """(M, r) of order NP: identity on the padded diagonal (k_make_PI), zero padding of A'A and of the right-hand side; AA: a (perturbed) padded A'A."""
    n, NP = pr.n, roundup(pr.n, 64)
    if AA is None:
        AA = padded_AA(pr)
    M = rho * AA
    M[:n, :n] += pr.P
    M[np.diag_indices(n)] += SIGMA
    M[np.arange(n, NP), np.arange(n, NP)] += 1.0
    r = np.zeros(NP)
    r[:n] = pr.M(rho) @ pr.xs
    return M, r


def padded_AA(pr):
    NP = roundup(pr.n, 64)
    AA = np.zeros((NP, NP))
    AA[:pr.n, :pr.n] = pr.AA
    return AA


def factor(M, dtype):
    """Lower Cholesky factor in the type, read from the lower triangle alone as on the device; None when it breaks down."""
    try:
        return sla.cholesky(M.astype(NPDT[dtype]), lower=True, check_finite=False)
    except np.linalg.LinAlgError:
        return None


def sweeps(L, r, n):
    """x = S'(S r) with S = inv(L) formed explicitly (the sweep matrix of build_sweep_matrix with one block); NaN where L is singular."""
    trtri, = sla.get_lapack_funcs(("trtri",), (L,))
    S, info = trtri(L, lower=1)
    if info != 0:
        return np.full(n, np.nan)
    S = np.tril(S)
    return (S.T @ (S @ r.astype(L.dtype)))[:n].astype(np.float64)


def restated_solve(pr, dtype, rho=RHO):
    M, r = padded(pr, rho)
    return sweeps(factor(M, dtype), r, pr.n)


def lapack_solve(pr, dtype, rho=RHO):
    T = NPDT[dtype]
    c = sla.cho_factor(pr.M(rho).astype(T), lower=True, check_finite=False)
    return sla.cho_solve(c, (pr.M(rho) @ pr.xs).astype(T), check_finite=False).astype(np.float64)


def xerr(x, pr):
    """max|x - x*| / max|x*|; inf when x is not finite."""
    e = np.abs(x - pr.xs).max() / np.abs(pr.xs).max()
    return float(e) if np.isfinite(e) else math.inf


def cpu_errors(pr, dtype, rho=RHO):
    """(e_alg, e_ref) of a problem."""
    return xerr(restated_solve(pr, dtype, rho), pr), xerr(lapack_solve(pr, dtype, rho), pr)


def all_problems():
    """(tag, problem, rho) of everything the bound is taken over."""
    for c in SINGLE:
        yield single_id(c), problem(c.n, c.m), RHO
        if c.n in RHO_SWITCH:
            yield single_id(c) + "-rho2", problem(c.n, c.m), RHO2
    for c in BATCH:
        for b, pr in enumerate(batch_problems(c)):
            yield f"{batch_id(c)}-qp{b}", pr, RHO


# Perturbations of the restated L and A'A: one lower 64 x 64 tile zeroed, or taken from its mirrored position (bi, bi - bj) -- the mirror image along its
# tile row inside the lower triangle, the axis k_gemm pairs tiles along; what a wrong id -> tile map or a wrong mirror tile of a pair would deliver.  A tile
# that is its own mirror image (bi = 2 bj) has no such perturbation.  (The reflection that maps diagonal tiles to diagonal tiles would not do: the diagonal
# tiles of L all carry pivots of about sqrt(d + 1 + ρ nnz), and exchanging two of them moves x by the 2 ... 8 % spread of those alone.)
def lower_tiles(nt):
    return [(bi, bj) for bi in range(nt) for bj in range(bi + 1)]


def listed_tiles(nt, count=1):
    """The first tile, the last, the last off-diagonal tile of the ragged block row, and the tiles dealt by the last tile-taking id of the two 1-D
    orders: A'A's (lower_tile_of, as a batch of ``count`` would use it) and the first update launch's of the chain (two block columns further in)."""
    tiles = {(0, 0), (nt - 1, nt - 1), (nt - 1, max(nt - 2, 0))}
    nids = lower_tile_ids(nt)
    tiles.add(next(t for t in (lower_tile_of(i, nids, nt) for i in reversed(range(nids))) if t is not None))
    steps = chol_steps("f32", 64 * nt, count)
    if steps:
        _, g, _, avoid, ids = steps[0]
        t = next((t for t in (chol_update_tile_of(i, avoid, g) for i in reversed(range(ids))) if t is not None), None)
        if t is not None:                                               # (g = 1: the diagonal workgroup alone)
            tiles.add((t[0] + 2, t[1] + 2))
    return sorted(tiles)


def perturbations(nt, tiles):
    return [(bi, bj, how) for (bi, bj) in tiles for how in ("zero", "mirror") if how == "zero" or bi != 2 * bj]


def perturbed(X, bi, bj, how):
    Y = X.copy()
    t = lambda i, j: (slice(64 * i, 64 * i + 64), slice(64 * j, 64 * j + 64))
    Y[t(bi, bj)] = 0.0 if how == "zero" else X[t(bi, bi - bj)]
    return Y


def moved_by(pr, which, bi, bj, how, L0=None):
    """Error of x when tile (bi, bj) of the restated L (which = "L"; L0: its unperturbed fp64 factor) or A'A ("AA") is perturbed, in fp64 (the
    arithmetic moves it by 1e-6 at the most); inf when the system breaks down, which the device would report."""
    if which == "L":
        L = perturbed(L0, bi, bj, how)
        r = padded(pr)[1]
    else:
        M, r = padded(pr, AA=perturbed(padded_AA(pr), bi, bj, how))
        L = factor(M, "f64")
        if L is None:
            return math.inf
    with np.errstate(all="ignore"):
        return xerr(sweeps(L, r, pr.n), pr)


# ---------------------------------------------------------------------------------------------------------------------
# The dispatch code, restated (file and line in the docstring above)
# ---------------------------------------------------------------------------------------------------------------------
def chol_scratch_elems(NP):
    return ((NP // 64 + 1) // 2) * 3 * 4096 + 64


def chol_scratch_fits(NP):
    return chol_scratch_elems(NP) <= NP * NP


def chol_update_ids(g, avoid):
    return 1 + (g * (g + 1) // 2 - 1) + ((g * (g + 1) // 2 - 1) // 7 + 2 if avoid else 0)


def chol_update_tile_of(id_, avoid, g):
    """(bi, bj) or None."""
    if id_ <= 0 or (avoid and id_ % 8 == 0):
        return None
    t = id_ - id_ // 8 if avoid else id_
    if t >= g * (g + 1) // 2:
        return None
    bi = (math.isqrt(8 * t + 1) - 1) // 2
    return bi, t - bi * (bi + 1) // 2


def lower_tile_ids(nt):
    return 8 * ((nt * (nt + 1) // 2 + 7) // 8)


def lower_tile_of(id_, nids, nt):
    """(bi, bj) or None (a padding id)."""
    S = 8
    t = (id_ & 7) * (nids >> 3) + (id_ >> 3)
    for I in range((nt + S - 1) // S):
        rows = min(S, nt - I * S)
        full = rows * I * S
        cnt = full + rows * (rows + 1) // 2
        if t < cnt:
            if t < full:
                J, r = divmod(t, rows * S)
                return I * S + r // S, J * S + r % S
            r, a = t - full, 0
            while r > a:
                r -= a + 1
                a += 1
            return I * S + a, I * S + r
        t -= cnt
    return None


def chol_steps(dtype, NP, batch=1):
    """The loop steps of the fused chain: (cb, g, nt, avoid, ids)."""
    out, nblk = [], NP // 64
    cb = 0
    while cb + 2 <= nblk:
        rem = NP - (cb + 2) * 64
        if rem <= 0:
            break
        g = rem // 64
        nt = g * (g + 1) // 2 - 1
        avoid = 1 if (batch == 1 and nt >= 256 and (dtype == "f32" or nt <= 1500)) else 0
        out.append((cb, g, nt, avoid, chol_update_ids(g, avoid)))
        cb += 2
    return out


def gemm_plan(Mr, Nc, ak, bk, lower_only, batch, ktri):
    """dict(pair, threshold, lower_map, ids, padding) of one gemm call."""
    ni, nj = Mr // 64, Nc // 64
    threshold = (not lower_only) and ktri != 0 and not (ak and bk) and ni * nj * batch >= 512
    pair = threshold and ((nj % 2 == 0) if ktri == 1 else (ni % 2 == 0))
    lower_map = bool(lower_only and ni == nj and ni >= 2 and ni * (ni + 1) // 2 * batch >= 512)
    ids = lower_tile_ids(ni) if lower_map else 0
    return dict(pair=bool(pair), threshold=bool(threshold), lower_map=lower_map, ids=ids, padding=ids - ni * (ni + 1) // 2 if lower_map else 0)


def sweep_fused_supported(dtype, NP):
    return 1024 <= NP <= 16 * 512 * VN[dtype]


def pick_nb(dtype, requested, NP):
    nb = requested if requested > 0 else (32768 if sweep_fused_supported(dtype, NP) else 4096)
    p = 64
    while p * 2 <= nb:
        p *= 2
    nb = p
    while nb > 64 and nb // 2 >= NP:
        nb //= 2
    return nb


def trsv_blocked_supported(dtype, NP, nb):
    vn, size = VN[dtype], 8 if dtype == "f64" else 4
    if nb not in (512 * vn, 256 * vn):
        return False
    nblk = (NP + nb - 1) // nb
    return nblk >= 2 and nblk * nb * size <= 144 * 1024


def sweep_gemms(NP, nb, batch, premul):
    """The triangular-operand products of build_sweep_matrix: (where, ktri, gemm_plan, launches) with where = full / ragged / premul."""
    out = []
    s = 64
    while s < nb:
        nfull = NP // (2 * s)
        if nfull > 0:
            z, launches = (nfull, 1) if batch == 1 else (batch, nfull)
            out.append(("full", 1, gemm_plan(s, s, True, False, False, z, 1), launches))
            out.append(("full", 2, gemm_plan(s, s, True, False, False, z, 2), launches))
        s2 = NP - nfull * 2 * s - s
        if s2 > 0:
            out.append(("ragged", 1, gemm_plan(s2, s, True, False, False, batch, 1), 1))
            out.append(("ragged", 2, gemm_plan(s2, s, True, False, False, batch, 2), 1))
        s *= 2
    if premul and batch == 1 and nb < NP:
        nblk = (NP + nb - 1) // nb
        for J in range(nblk - 1):
            out.append(("premul", 3, gemm_plan(nb, NP - (J + 1) * nb, False, True, False, 1, 3), 1))
        for J in range(1, nblk):
            out.append(("premul", 2, gemm_plan(min(nb, NP - J * nb), J * nb, True, False, False, 1, 2), 1))
    return out


def branches(n, m, dtype, count=1, trsv=0, rho_switch=False):
    """The branches of the setup chain that a handle of this shape reaches."""
    NP, MP = roundup(n, 64), roundup(m, 64)
    nblk, b = NP // 64, set()
    # Cholesky
    if not chol_scratch_fits(NP):
        b.add("chol:64col")
    else:
        b.update({"chol:fused", "chol:nblk_odd_tail" if nblk % 2 else "chol:nblk_even"})
        steps = chol_steps(dtype, NP, count)
        if not steps:
            b.add("chol:no_loop_step")
        for (_, g, nt, avoid, ids) in steps:
            b.add("chol:update_g1" if g == 1 and ids == 1 else "chol:update_g>=2")
        av = [s[3] for s in steps]
        if steps and count == 1:
            par = "odd" if nblk % 2 else "even"
            if not any(av):
                b.add("avoid:never")
            elif av[0] and sum(av) == 1:
                b.add(f"avoid:first_step_only_{par}")
            elif av[0]:
                b.add("avoid:on_then_off")
            else:
                b.add("avoid:f64_unavoided_then_avoided")
            if dtype == "f32" and any(s[2] > 1500 and s[3] for s in steps):
                b.add("avoid:f32_beyond_1500")
    # A'A
    gg = gemm_plan(NP, NP, False, False, True, count, 0)
    tag = "_batch" if count > 1 else ""
    b.add(("gg:1d" + ("_padding" if gg["padding"] else "_no_padding") if gg["lower_map"] else "gg:2d") + tag)
    if rho_switch:
        b.add("refactor:cached_gg")
    # sweep matrix
    nb = pick_nb(dtype, trsv, NP)
    premul = count == 1 and trsv_blocked_supported(dtype, NP, nb)
    calls = sweep_gemms(NP, nb, count, premul)
    if not any(w != "premul" for (w, _, _, _) in calls):
        b.add("dbl:none")
    for (where, ktri, plan, launches) in calls:
        if where == "full":
            b.add("dbl:full_z" if count == 1 else "dbl:full_hostloop")
        elif where == "ragged":
            b.add("dbl:ragged" if count == 1 else "dbl:ragged_batch")
        b.add(("pair" if plan["pair"] else "odd" if plan["threshold"] else "small") + f":{where}_ktri{ktri}")
    if nb < NP:
        b.add("dbl:stops_below_NP")
        b.add("premul:on" if premul else "sweep:multi_launch")
        if premul and NP % nb:
            b.add("premul:ragged_last_row")
    else:
        b.add("sweep:one_block")
    if count > 1 and gg["lower_map"] and "dbl:full_hostloop" in b:
        b.add("batch:1d_order_with_hostloop")
    return b


def table_branches():
    """The union over the whole table, both types."""
    b = set()
    for dt in DTYPES:
        for c in SINGLE:
            b |= branches(c.n, c.m, dt, rho_switch=c.n in RHO_SWITCH)
            for nbq in TRSV.get(c.n, {}).get(dt, ()):
                b |= branches(c.n, c.m, dt, trsv=nbq)
        for c in BATCH:
            b |= branches(c.n, c.m, dt, count=c.count)
    return b


# every branch named by the band list in the docstring, both sides of every threshold
REQUIRED = {
    "chol:64col", "chol:fused", "chol:nblk_even", "chol:nblk_odd_tail", "chol:no_loop_step", "chol:update_g1", "chol:update_g>=2",
    "avoid:never", "avoid:first_step_only_odd", "avoid:first_step_only_even", "avoid:on_then_off", "avoid:f64_unavoided_then_avoided", "avoid:f32_beyond_1500",
    "gg:2d", "gg:1d_no_padding", "gg:1d_padding", "gg:2d_batch", "gg:1d_padding_batch", "refactor:cached_gg",
    "dbl:none", "dbl:full_z", "dbl:full_hostloop", "dbl:ragged", "dbl:ragged_batch", "dbl:stops_below_NP", "batch:1d_order_with_hostloop",
    "small:full_ktri1", "small:full_ktri2", "pair:full_ktri1", "pair:full_ktri2",
    "small:ragged_ktri1", "small:ragged_ktri2", "pair:ragged_ktri1", "pair:ragged_ktri2", "odd:ragged_ktri2",
    "premul:on", "premul:ragged_last_row", "small:premul_ktri3", "pair:premul_ktri3", "small:premul_ktri2", "pair:premul_ktri2",
    "sweep:multi_launch", "sweep:one_block",
}
