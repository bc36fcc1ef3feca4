"""The case table of tests/test_gpu_small_bands.py (GPU) and tests/test_small_bands_cpu.py (CPU guards): one case per geometry band of the
single-launch small-problem kernels of k_small.hip -- the LDS-vector kernel k_admm_small<T, ST, LM> and the register kernel
k_admm_small_reg<T, NB, MB> with its batch twin -- in both types, held to the structured fp64 reference of tests/width_band_cases.py.  Plain
importable helper, no device needed.

The bands.  NP = roundup(n, 64), MP = roundup(m, 64).  The handle reports ``sweepVariant == 4`` for the single launch (asserted on the GPU); the
rest is read off the dispatch code, restated below as ``small_route`` and asserted against every case's claim by the CPU guards:
  domain   k_small.hip admm_small_supported: m >= 1, NP <= 512, MP <= 2048, small_lds_bytes <= 150 KiB and (2 MP NP + NP^2) sizeof(T) <= 1.25 MiB.
  reg      admm_small: NP in {64, 128} with MP / 64 <= mb_max = 2 (fp64) / 4 (fp32) -> k_admm_small_reg<T, NP / 64, MP / 64>, 512 threads; the same rule
           (admm_small_batch_supported) sends a batch to k_admm_small_reg_batch, one workgroup per QP.  QPS_SMALL_REG=0 switches both off.
  lds      otherwise k_admm_small<T, ST, LM>: LM (A with row stride NP + 1 and S copied into LDS) when small_lds_bytes + small_lds_mat_bytes
           <= 158 KiB and QPS_SMALL_LDSMAT is not 0; ST = 512 while MP NP <= 65536, else 1024 (QPS_SMALL_THREADS overrides: <= 256 -> 256, <= 512 -> 512).
  products gemv_cols_lds<T, ST> walks its columns in j0 passes of ST; a pass of nc columns runs J = the power of two >= max(nc, 64) lanes along the
           columns and G = ST / J row groups.  A'w, the two triangular sweeps, P x and A'y have NP <= 512 <= ST columns: one pass, J = J(NP).
           A x~ (and A x of the check) has MP columns: two passes when MP > ST, the second with its own J.  With LM, A x~ is gemv_rows_ldsmat instead:
           R = the power of two >= min(max(MP, 64), ST) lanes along the rows, PARTS = ST / R column ranges, ceil(MP / R) row blocks.
A route is written (kernel, ST, LM, J of the n-wide products, passes of the A x~ product or None with LM); a register route ("reg", NB, MB).

Shapes.  "entry" shapes are ragged: n = NP - 60, m = MP - 60, four real columns and four real rows in the last 64-block, so the second pass of a
two-pass product holds four real entries; "full" shapes fill the named dimension.  ``B`` is the first column of the last 64-block; for B > 0 the
columns >= B are weighted as in width_band_cases.Family.  The single-handle cases with B > 0 and no ``stream`` ARE Family(n, B, m=m); the others
(B = 0: one column block, nothing to weight; the batch members; draws replaced because their active share missed the window) are ``Member``s, which
duck-type Family over the same distributions drawn from make_rng(2718, stream), ``stream`` = (stream, q scale).  The window is a condition on the
inputs (10 % ... 60 % of the rows at a bound after the K iterations, CPU guard): with four variables and hundreds of rows the base distributions
leave no row at a bound, so those members scale q by 4 ... 256; full n = 512 with four rows scales it by 0.25; members with four rows take a
stream that leaves one or two rows active.  Batch members are make_rng(2718, 100 + member), member = 0, 1, 2 (BATCH_MEMBERS: 1, 2, 3 at (68, 4), where
member 0 has three of four rows active).  Every run: K = 20, a check every 10, rho = 0.1, sigma and alpha of the reference signature, the member's
non-zero x0, eps = 0.

Bounds.  fp64: TOL["f64"].  fp32: per run and quantity min(100 x the fp32 emulation's own error against the fp64 reference, TOL["f32"]), the rule of
width_band_cases.bounds; the emulation figures are recorded in EMU_F32 (tests/test_small_bands_cpu.py reproduces them within a factor 2).  They are
taken with BLAS held to one thread where threadpoolctl is installed: at n >= 260 the split of a product over threads moves the residual figures
by more than that factor.

Measured on an MI355X (printed before every assertion, run with -s; largest figure of each group against its bound).  No run came nearer than 0.27 of
a bound and none needed a raised fp32 bound.  51 tests in 3.7 s, 2.1 s of it the three knob children.
  LDS fp64        x 5.5e-14, z 2.0e-13, y 2.2e-14, resPrim 4.6e-14, resDual 1.3e-12 against 1e-9 (y 1e-8); the three adaptive runs (one refactor at
                  iteration 11 each, rhoFinal equal to 12 digits): x 2.0e-13, z 8.1e-13, resDual 1.2e-12.
  LDS fp32        x 2.5e-6, z 4.8e-6, y 4.0e-7, resPrim 2.5e-6, resDual 1.5e-5; nearest to its bound: resDual 5.7e-6 against 3.0e-5 at (260, 196).
  register fp64   x 9.9e-15, z 2.1e-13, y 3.1e-14, resPrim 2.9e-13, resDual 5.7e-13.
  register fp32   x 8.1e-7, z 2.1e-6, y 4.5e-7, resPrim 4.7e-7, resDual 7.7e-6; nearest: resPrim 1.3e-7 against 6.0e-7 at (60, 132).  Adaptive run at
                  (68, 196): z 4.9e-6 against 1.9e-4, one refactor, rho 0.3015371 against the reference's 0.3015358.
  batch fp64      x 5.2e-15, z 2.6e-14, y 6.1e-15, resPrim 1.3e-14, resDual 9.6e-13; adaptive (2, 2): member 0 refactors once (rho 0.2145), 1 and 2 do not.
  batch fp32      x 6.2e-7, z 8.7e-7, y 3.7e-7, resPrim 5.8e-7, resDual 8.7e-6; nearest: resPrim 5.8e-7 against 2.1e-6 at (68, 132) member 0.
  outside         fp64 z 1.4e-14; fp32 x 6.4e-7 against 2.6e-5; neither reports sweepVariant 4.
  knob forms      fp64 resDual 5.3e-13; fp32 resDual 2.9e-6 against 1.2e-4, nearest resPrim 4.1e-7 against 6.3e-6 (QPS_SMALL_REG=0 at (68, 4)).
  repeat          fp64 (68, 132) on the LDS kernel and fp32 (68, 196) on the register kernel: the second solve equals the first bit for bit.
Two deliberate breaks, each run once in a throw-away build: gemv_cols_lds leaving after its first j0 pass fails exactly the seven two-pass cases; nget of
small_reg_body reading block 0 for i >= 64 fails exactly the fourteen NB = 2 register cases (eight single, six batch)."""
import contextlib
import math
from collections import namedtuple

import numpy as np

import width_band_cases as W
from loop_param_cases import TOL
from quadraticprogramsolver_amd.generator import make_rng
from width_band_cases import ADMM_FCTR, ADMM_KEYS, ALPHA, K, PERIOD, RHO, SIGMA, DenseF32, Family, Structured, admm_loop, errors, roundup  # noqa: F401

try:                                                                   # the emulation's rounding depends on how BLAS splits a product over its threads
    from threadpoolctl import threadpool_limits
except ImportError:                                                    # (without the package the figures are those of the default thread count)
    def threadpool_limits(limits=None):
        return contextlib.nullcontext()

SZ = {"f64": 8, "f32": 4}
MB_MAX = {"f64": 2, "f32": 4}                                          # admm_small: mb_max
REG_NP = (64, 128)
LDS_LIMIT, LM_LIMIT, BYTES_LIMIT, ST_SWITCH = 150 * 1024, 158 * 1024, 1.25 * 1024 * 1024, 65536
NP_MAX, MP_MAX = 512, 2048
COUNT = 3                                                              # QPs of a batch case


# ---------------------------------------------------------------------------------------------------------------------
# The dispatch code of k_small.hip, restated
# ---------------------------------------------------------------------------------------------------------------------
def small_lds_bytes(dtype, NP, MP):
    return SZ[dtype] * (6 * NP + 7 * MP + 1024)


def small_lds_mat_bytes(dtype, NP, MP):
    return SZ[dtype] * (MP * (NP + 1) + NP * NP)


def admm_small_supported(dtype, n, m):
    NP, MP = roundup(n, 64), roundup(m, 64)
    if m < 1 or NP > NP_MAX or MP > MP_MAX or small_lds_bytes(dtype, NP, MP) > LDS_LIMIT:
        return False
    return (2.0 * MP * NP + float(NP) * NP) * SZ[dtype] <= BYTES_LIMIT


def reg_instantiation(dtype, NP, MP, reg=True):
    """(NB, MB) of the register kernel, or None: the rule of admm_small and of admm_small_batch_supported."""
    if reg and MP >= 64 and NP in REG_NP and MP // 64 <= MB_MAX[dtype]:
        return NP // 64, MP // 64
    return None


def admm_small_batch_supported(dtype, n, m, reg=True):
    return reg_instantiation(dtype, roundup(n, 64), roundup(m, 64), reg) is not None


def cols_plan(ST, ncols):
    """gemv_cols_lds<T, ST> on ``ncols`` columns: [(J, G, nc)] per j0 pass."""
    out = []
    for j0 in range(0, ncols, ST):
        nc = min(ncols - j0, ST)
        J = 64
        while J < nc:
            J <<= 1
        out.append((J, ST // J, nc))
    return out


def rows_plan(ST, nrows):
    """gemv_rows_ldsmat<T, ST> on ``nrows`` rows: (R, PARTS, row blocks)."""
    R = 64
    while R < nrows and R < ST:
        R <<= 1
    return R, ST // R, -(-nrows // R)


Route = namedtuple("Route", "kernel ST LM J passes n_plan ax_plan")   # n_plan: cols_plan of the n-wide products; ax_plan: cols_plan / rows_plan of A x~


def small_route(dtype, n, m, reg=True, ldsmat=True, threads=0):
    """What admm_small launches for a single handle of (n, m), or None outside admm_small_supported.  reg / ldsmat / threads: QPS_SMALL_REG,
    QPS_SMALL_LDSMAT, QPS_SMALL_THREADS.  A register route is ("reg", NB, MB)."""
    if not admm_small_supported(dtype, n, m):
        return None
    NP, MP = roundup(n, 64), roundup(m, 64)
    inst = reg_instantiation(dtype, NP, MP, reg)
    if inst:
        return ("reg",) + inst
    lds = small_lds_bytes(dtype, NP, MP)
    lm = bool(ldsmat) and lds + small_lds_mat_bytes(dtype, NP, MP) <= LM_LIMIT
    th = threads if threads > 0 else (512 if MP * NP <= ST_SWITCH else 1024)
    ST = 256 if th <= 256 else 512 if th <= 512 else 1024
    n_plan = cols_plan(ST, NP)
    ax_plan = rows_plan(ST, MP) if lm else cols_plan(ST, MP)
    assert len(n_plan) == 1                                            # NP <= 512: the n-wide products never take a second pass ...
    assert ST >= 512 or NP <= ST                                       # ... at the default widths; a 256-thread knob run must keep NP <= 256
    return Route("lds", ST, int(lm), n_plan[0][0], None if lm else len(ax_plan), n_plan, ax_plan)


def signature(route):
    return route if route[0] == "reg" else tuple(route[:5])


# ---------------------------------------------------------------------------------------------------------------------
# The cases.  route: the claim.  stream: None -> Family(n, B, m=m) (needs B > 0), else (stream, q scale) of Member(n, m, B, stream, qscale).
# ---------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "dtype n m kind NP MP B route stream")


def _lds(dtype, NP, MP, route, full_n=False, full_m=False, stream=None):
    n, m = (NP if full_n else NP - 60), (MP if full_m else MP - 60)
    B = NP - 64
    if B == 0 and stream is None:
        stream = (10, 1.0)
    return Case(dtype, n, m, "full" if (full_n or full_m) else "entry", NP, MP, B, ("lds",) + route, stream)


LDS_CASES = [
    _lds("f64", 64, 192, (512, 1, 64, None), stream=(10, 64.0)),
    _lds("f64", 64, 320, (512, 0, 64, 1), stream=(10, 64.0)),
    _lds("f64", 64, 576, (512, 0, 64, 2), stream=(10, 64.0)),
    _lds("f64", 64, 1088, (1024, 0, 64, 2), stream=(10, 256.0)),
    _lds("f64", 64, 1216, (1024, 0, 64, 2), full_n=True, full_m=True, stream=(10, 16.0)),    # the last supported shape of NP = 64 in fp64
    _lds("f64", 128, 192, (512, 0, 128, 1)),
    _lds("f64", 128, 576, (1024, 0, 128, 1), stream=(10, 4.0)),
    _lds("f64", 192, 64, (512, 0, 256, 1), stream=(11, 1.0)),                               # nc = 192 < J = 256
    _lds("f64", 256, 192, (512, 0, 256, 1), full_n=True),
    _lds("f64", 320, 64, (512, 0, 512, 1)),
    _lds("f32", 64, 320, (512, 1, 64, None), stream=(10, 64.0)),
    _lds("f32", 64, 512, (512, 0, 64, 1), stream=(10, 64.0)),
    _lds("f32", 64, 576, (512, 0, 64, 2), stream=(10, 64.0)),
    _lds("f32", 64, 1088, (1024, 0, 64, 2), stream=(10, 256.0)),
    _lds("f32", 64, 2048, (1024, 0, 64, 2), full_m=True, stream=(11, 256.0)),
    _lds("f32", 128, 320, (512, 0, 128, 1)),
    _lds("f32", 128, 576, (1024, 0, 128, 1), stream=(10, 4.0)),
    _lds("f32", 128, 1088, (1024, 0, 128, 2), stream=(10, 16.0)),
    _lds("f32", 192, 64, (512, 0, 256, 1), stream=(11, 1.0)),
    _lds("f32", 256, 320, (1024, 0, 256, 1)),
    _lds("f32", 512, 64, (512, 0, 512, 1), full_n=True, stream=(15, 0.25)),
    _lds("f32", 320, 256, (1024, 0, 512, 1)),
]


def _reg(dtype, NB, MB, full=False, stream=None):
    n = 64 * NB if full else (60 if NB == 1 else 68)
    m = 64 * MB if full else 64 * MB - 60
    B = 64 * (NB - 1)
    if B == 0 and stream is None:
        stream = (20, 1.0)
    if (NB, MB) == (2, 4) and not full:
        stream = (11, 4.0)                                             # the fp32 adaptive register run: the base draw's first proposal stays inside the band
    return Case(dtype, n, m, "full" if full else "entry", 64 * NB, 64 * MB, B, ("reg", NB, MB), stream)


REG_INSTANCES = [("f64", nb, mb) for nb in (1, 2) for mb in (1, 2)] + [("f32", nb, mb) for nb in (1, 2) for mb in (1, 2, 3, 4)]
REG_CASES = [_reg(*i) for i in REG_INSTANCES] + [_reg("f64", 2, 2, full=True), _reg("f32", 2, 4, full=True)]
BATCH_CASES = [_reg(*i) for i in REG_INSTANCES]                           # count = COUNT members each: make_rng(2718, 100 + member)
BATCH_MEMBERS = {"f64-n68-m4": (1, 2, 3), "f32-n68-m4": (1, 2, 3)}                                                     # case id -> member numbers, where (0, 1, 2) missed the active-share window
OUTSIDE_CASES = [                                                      # just outside admm_small_supported: the multi-launch loop, same bounds
    Case("f64", 260, 68, "outside", 320, 128, 256, None, None),
    Case("f32", 452, 132, "outside", 512, 192, 448, None, None),
]
SINGLE_CASES = LDS_CASES + REG_CASES


def case_id(c):
    return f"{c.dtype}-n{c.n}-m{c.m}"


def find(cases, dtype, n, m):
    return next(c for c in cases if (c.dtype, c.n, c.m) == (dtype, n, m))


# adaptive runs (adptRho, fctrRho = ADMM_FCTR): the proposal of the first check must cross the band (CPU guard)
ADAPTIVE_SINGLE = [("f64", 4, 260), ("f64", 4, 132), ("f64", 4, 1028), ("f32", 68, 196)]   # LM-off 512 threads; LM; two-pass 1024 threads; register NB = 2
ADAPTIVE_BATCH = ("f64", 68, 68)                                       # register (2, 2), batch form
REPEAT_SINGLE = [("f64", 68, 132), ("f32", 68, 196)]                   # one LDS case, one register case: a second solve on the same handle, bit for bit

# knob-only forms: (environment, [(dtype, n, m, claimed route under the knobs)]); every shape is a case above, held to that case's reference and bounds
KNOB_RUNS = [
    ({"QPS_SMALL_REG": "0"}, [("f32", 68, 4, ("lds", 512, 1, 128, None)), ("f64", 68, 68, ("lds", 512, 0, 128, 1))]),
    ({"QPS_SMALL_LDSMAT": "0"}, [("f64", 4, 132, ("lds", 512, 0, 64, 1)), ("f32", 4, 260, ("lds", 512, 0, 64, 1))]),
    ({"QPS_SMALL_REG": "0", "QPS_SMALL_THREADS": "256"}, [("f32", 4, 260, ("lds", 256, 1, 64, None)), ("f64", 132, 4, ("lds", 256, 0, 256, 1))]),
]


def solve_params(**extra):
    """The scalars of every run, in the oracle's spelling (loop_param_cases.api_kw turns them into the package's keywords)."""
    return dict(numIterations=K, numItrConv=PERIOD, epsAbs=0.0, epsRel=0.0, rho=RHO, sigma=SIGMA, alpha=ALPHA, **extra)


def knob_kw(env):
    return dict(reg=env.get("QPS_SMALL_REG", "1") != "0", ldsmat=env.get("QPS_SMALL_LDSMAT", "1") != "0", threads=int(env.get("QPS_SMALL_THREADS", "0")))


# ---------------------------------------------------------------------------------------------------------------------
# Problem data
# ---------------------------------------------------------------------------------------------------------------------
class Member:
    """Duck-types width_band_cases.Family (d, U, A, q, l, u, x0, n, m, B, _cache) over the same distributions, drawn from make_rng(2718, stream) at the
    member's own size.  B = 0 (a single column block): no column is weighted."""
    dense_P = Family.dense_P

    def __init__(self, n, m, B, stream, qscale=1.0, weight=W.WEIGHT):
        rng = make_rng(2718, stream)
        assert 0 <= B < n
        self.n, self.m, self.B = n, m, B
        wcol = np.where(np.arange(n) >= B, weight, 1.0) if B > 0 else np.ones(n)
        self.d = 0.5 + rng.random(n)
        self.U = rng.standard_normal((n, 8)) * (wcol / math.sqrt(n))[:, None]
        self.A = np.asfortranarray(rng.standard_normal((n, m)).T * (wcol / math.sqrt(n))[None, :])
        self.q, self.x0 = qscale * rng.standard_normal(n), 0.3 * rng.standard_normal(n)
        self.l, self.u = -1.05 * (0.5 + rng.random(m)), 1.05 * (0.5 + rng.random(m))
        self.me = None
        self._cache = {}


_members = {}


def member(case, k=None):
    """The problem of a single-handle case (k None) or member k of a batch case; cached, treat as read-only."""
    key = (case_id(case), case.stream, k)
    if key not in _members:
        if k is not None:
            _members[key] = Member(case.n, case.m, case.B, 100 + BATCH_MEMBERS.get(case_id(case), (0, 1, 2))[k])
        elif case.stream is None:
            _members[key] = Family(case.n, case.B, m=case.m)
        else:
            _members[key] = Member(case.n, case.m, case.B, *case.stream)
    return _members[key]


def without_last_row(f):
    """A copy of a member whose last real row of A is zero: what a kernel computes that drops that row."""
    g = object.__new__(Member)
    g.__dict__.update(f.__dict__)
    g.A = f.A.copy(order="F")
    g.A[f.m - 1, :] = 0.0
    g._cache = {}
    return g


_refs = {}


def reference(case, k=None, adpt=False):
    """admm_loop(Structured(member)) of a case, computed once and shared; treat as read-only."""
    key = (case_id(case), case.stream, k, adpt)
    if key not in _refs:
        _refs[key] = admm_loop(Structured(member(case, k)), adpt=adpt, fctr=ADMM_FCTR)
    return _refs[key]


def emu_key(case, k=None, adpt=False):
    return case_id(case) + ("" if k is None else f"-b{k}") + ("-adaptive" if adpt else "")


def emulation_error(case, k=None, adpt=False):
    """The fp32 emulation of a case against its fp64 reference: the figures recorded in EMU_F32."""
    with threadpool_limits(limits=1):
        return errors(admm_loop(DenseF32(member(case, k)), adpt=adpt, fctr=ADMM_FCTR), reference(case, k, adpt), ADMM_KEYS)


def bounds(case, k=None, adpt=False):
    """The bound of every compared quantity of a case (of member k of a batch case)."""
    if case.dtype == "f64":
        return dict(TOL["f64"])
    emu = EMU_F32[emu_key(case, k, adpt)]
    return {q: min(100.0 * emu[q], TOL["f32"][q]) for q in TOL["f32"]}


def fp32_runs():
    """Every (case, member, adaptive) whose bound comes from the emulation: the keys of EMU_F32."""
    out = [(c, None, False) for c in SINGLE_CASES + OUTSIDE_CASES if c.dtype == "f32"]
    out += [(c, k, False) for c in BATCH_CASES if c.dtype == "f32" for k in range(COUNT)]
    out += [(find(SINGLE_CASES, *a), None, True) for a in ADAPTIVE_SINGLE if a[0] == "f32"]
    return out


# Error of the fp32 emulation against the fp64 reference (``emulation_error``), recorded on the CPU once per run.
EMU_F32 = {
    "f32-n4-m260": dict(x=2.31e-07, z=1.31e-06, y=8.98e-08, resPrim=3.85e-07, resDual=1.19e-06),
    "f32-n4-m452": dict(x=1.00e-06, z=1.07e-06, y=1.31e-07, resPrim=6.93e-07, resDual=1.82e-06),
    "f32-n4-m516": dict(x=1.30e-06, z=1.81e-06, y=2.12e-07, resPrim=1.17e-06, resDual=1.25e-06),
    "f32-n4-m1028": dict(x=5.80e-07, z=1.92e-06, y=1.90e-07, resPrim=9.50e-07, resDual=1.02e-05),
    "f32-n4-m2048": dict(x=1.78e-06, z=2.69e-06, y=1.73e-07, resPrim=3.25e-06, resDual=1.10e-05),
    "f32-n68-m260": dict(x=3.56e-07, z=4.38e-07, y=1.24e-07, resPrim=8.57e-08, resDual=1.14e-06),
    "f32-n68-m516": dict(x=4.92e-07, z=2.03e-06, y=1.23e-07, resPrim=4.99e-07, resDual=2.32e-06),
    "f32-n68-m1028": dict(x=1.92e-06, z=3.23e-06, y=1.92e-07, resPrim=1.28e-06, resDual=4.81e-05),
    "f32-n132-m4": dict(x=2.23e-07, z=6.54e-07, y=1.50e-07, resPrim=7.78e-07, resDual=7.09e-07),
    "f32-n196-m260": dict(x=6.55e-07, z=5.94e-07, y=1.56e-07, resPrim=1.63e-07, resDual=2.70e-06),
    "f32-n512-m4": dict(x=2.19e-06, z=6.43e-06, y=9.35e-08, resPrim=1.75e-06, resDual=2.72e-07),
    "f32-n260-m196": dict(x=1.80e-07, z=6.75e-07, y=2.29e-07, resPrim=1.01e-07, resDual=3.02e-07),
    "f32-n60-m4": dict(x=3.13e-07, z=2.76e-07, y=6.15e-08, resPrim=2.20e-07, resDual=1.27e-07),
    "f32-n60-m68": dict(x=4.17e-07, z=3.42e-07, y=1.80e-07, resPrim=6.67e-08, resDual=2.46e-07),
    "f32-n60-m132": dict(x=2.69e-07, z=3.13e-07, y=2.15e-07, resPrim=6.01e-09, resDual=1.13e-07),
    "f32-n60-m196": dict(x=2.83e-07, z=6.45e-07, y=1.83e-07, resPrim=2.50e-07, resDual=8.62e-08),
    "f32-n68-m4": dict(x=2.73e-07, z=3.30e-07, y=1.72e-07, resPrim=6.27e-08, resDual=1.23e-06),
    "f32-n68-m68": dict(x=3.61e-07, z=3.73e-07, y=1.76e-07, resPrim=7.30e-08, resDual=6.17e-07),
    "f32-n68-m132": dict(x=3.46e-07, z=5.27e-07, y=1.39e-07, resPrim=1.69e-07, resDual=4.04e-06),
    "f32-n68-m196": dict(x=7.24e-07, z=1.19e-06, y=1.71e-07, resPrim=6.47e-07, resDual=6.78e-06),
    "f32-n128-m256": dict(x=3.27e-07, z=2.02e-06, y=3.67e-07, resPrim=4.28e-07, resDual=7.34e-07),
    "f32-n452-m132": dict(x=2.64e-07, z=7.46e-07, y=1.83e-07, resPrim=3.49e-07, resDual=3.51e-06),
    "f32-n60-m4-b0": dict(x=4.36e-07, z=3.20e-07, y=6.87e-08, resPrim=4.20e-07, resDual=1.16e-06),
    "f32-n60-m4-b1": dict(x=3.77e-07, z=2.57e-07, y=8.82e-08, resPrim=2.49e-07, resDual=2.25e-07),
    "f32-n60-m4-b2": dict(x=2.85e-07, z=8.19e-08, y=1.13e-07, resPrim=4.45e-08, resDual=3.47e-07),
    "f32-n60-m68-b0": dict(x=1.74e-07, z=2.75e-07, y=9.49e-08, resPrim=1.03e-07, resDual=1.42e-07),
    "f32-n60-m68-b1": dict(x=2.56e-07, z=4.09e-07, y=1.22e-07, resPrim=7.52e-08, resDual=9.16e-08),
    "f32-n60-m68-b2": dict(x=4.09e-07, z=5.32e-07, y=2.18e-07, resPrim=2.16e-07, resDual=3.56e-07),
    "f32-n60-m132-b0": dict(x=2.23e-07, z=3.77e-07, y=2.06e-07, resPrim=8.63e-08, resDual=3.23e-07),
    "f32-n60-m132-b1": dict(x=1.89e-07, z=2.46e-07, y=1.90e-07, resPrim=1.10e-07, resDual=1.29e-08),
    "f32-n60-m132-b2": dict(x=3.57e-07, z=1.42e-06, y=2.24e-07, resPrim=4.19e-08, resDual=3.52e-07),
    "f32-n60-m196-b0": dict(x=4.63e-07, z=3.56e-07, y=1.76e-07, resPrim=1.79e-07, resDual=2.25e-07),
    "f32-n60-m196-b1": dict(x=4.15e-07, z=4.16e-07, y=2.23e-07, resPrim=1.12e-07, resDual=1.03e-07),
    "f32-n60-m196-b2": dict(x=2.07e-07, z=3.16e-07, y=2.14e-07, resPrim=2.98e-08, resDual=2.65e-07),
    "f32-n68-m4-b0": dict(x=1.34e-07, z=6.58e-07, y=1.31e-07, resPrim=1.86e-07, resDual=2.22e-06),
    "f32-n68-m4-b1": dict(x=2.89e-07, z=3.83e-08, y=2.34e-07, resPrim=7.32e-08, resDual=2.97e-06),
    "f32-n68-m4-b2": dict(x=3.18e-07, z=8.27e-07, y=3.62e-07, resPrim=2.49e-07, resDual=2.62e-06),
    "f32-n68-m68-b0": dict(x=2.09e-07, z=3.54e-07, y=1.60e-07, resPrim=1.76e-07, resDual=9.16e-08),
    "f32-n68-m68-b1": dict(x=4.34e-07, z=5.82e-07, y=2.88e-07, resPrim=8.99e-08, resDual=2.56e-07),
    "f32-n68-m68-b2": dict(x=3.87e-07, z=2.14e-07, y=1.29e-07, resPrim=1.36e-07, resDual=4.51e-06),
    "f32-n68-m132-b0": dict(x=4.18e-07, z=3.73e-07, y=2.37e-07, resPrim=2.13e-08, resDual=1.85e-06),
    "f32-n68-m132-b1": dict(x=3.32e-07, z=3.01e-07, y=2.19e-07, resPrim=1.74e-07, resDual=3.62e-06),
    "f32-n68-m132-b2": dict(x=3.38e-07, z=4.32e-07, y=1.56e-07, resPrim=1.29e-07, resDual=1.06e-06),
    "f32-n68-m196-b0": dict(x=2.21e-07, z=3.48e-07, y=2.89e-07, resPrim=2.58e-08, resDual=5.26e-07),
    "f32-n68-m196-b1": dict(x=3.53e-07, z=5.57e-07, y=2.53e-07, resPrim=1.65e-07, resDual=4.49e-06),
    "f32-n68-m196-b2": dict(x=3.49e-07, z=4.25e-07, y=2.25e-07, resPrim=1.47e-07, resDual=6.26e-06),
    "f32-n68-m196-adaptive": dict(x=6.02e-07, z=1.94e-06, y=6.53e-07, resPrim=1.97e-07, resDual=9.54e-06),
}
