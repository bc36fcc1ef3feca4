"""The case table of tests/test_capi_errors_cpu.py (CPU) and tests/test_gpu_capi_gates.py (GPU): named argument recipes for the refusals of the C boundary
(csrc/qps_capi.hip), and the function that recorded tests/golden/capi_errors.json.  The fixture holds, per case, the status and the full qps_last_error
text that the library gave BEFORE the boundary was refactored; the tests only compare.  Plain importable helper.

A recipe is a base argument set of one entry point plus one or two *faults* (small edits of that set).  Every creator lists its faults in the order in
which it tests for them; the table holds each fault alone and every adjacent pair together, so that the order is pinned too (the pair must answer as
its first fault alone does).  Shapes are the smallest that carry the fault: n = 3, m = 2, count = 2; n = 70 where an asymmetric entry has to sit
outside the first 64-tile.

Left out, with the reason:
  * "n beyond the limit of the whole-factor explicit inverse" (dense shared batch): the finiteness walk over P comes first and needs n = 16385 (2 GiB).
  * "more than 2^31 non-zeros" and the n > 2e9 "problem too large" of the sparse ProxQP creator: the CSC walk comes first and needs that many entries.
  * "problem too large to densify" of qps_create_csc: tested after the device, see tests/test_gpu_capi_gates.py.

Record again (only from a library whose answers are the reference):  python tests/capi_error_cases.py record [--lib PATH]          (no device)
                                                                      python tests/capi_error_cases.py record-device [--lib PATH]   (on the GPU)"""
import ctypes as C
import json
import os
import sys
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "capi_errors.json")
DP, IP, I32P = C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
NO_MESSAGE = "invalid handle"        # what prime() leaves behind: the text of a case whose entry point sets no message of its own

# name: the fixture key; call(L, args) -> (status, handle or None, extra or None); args: () -> dict; device: a well-formed call that reaches the device
# check (status 7 without a GPU; with one, what the fixture's "with_device" section holds and the handle is destroyed); first: for an order-pinning pair
# the name of the case that holds its first fault alone; env: environment of the call
Case = namedtuple("Case", "name call args device first env")
CASES = []
CREATORS = ("qps_create_dense", "qps_create_csc", "qps_create_dense_batch", "qps_create_dense_shared_batch", "qps_create_csc_shared_batch",
            "qps_proxqp_create_dense", "qps_proxqp_create_csc")
PROXQP_FINITENESS = ("nan_P", "nan_A", "nan_C", "nan_q")                # qps_proxqp_create_dense asks for the device BEFORE these


def ptr(a):
    if a is None:
        return None
    return a.ctypes.data_as({np.dtype(np.float64): DP, np.dtype(np.int64): IP, np.dtype(np.int32): I32P}[a.dtype])


def prime(L):
    """Leaves a known text in the thread's last-error slot (an entry point that sets none of its own is then recorded with this one)."""
    L.qps_linsys_set_cg(None, 0.0, 0)


def message(L):
    return (L.qps_last_error(None) or b"").decode("utf-8", "replace")


# ---------------------------------------------------------------------------------------------------------------------
# base problems
# ---------------------------------------------------------------------------------------------------------------------
def spd(n):
    M = np.random.default_rng(n).standard_normal((n, n))
    return np.asfortranarray(0.5 * ((M.T @ M + n * np.eye(n)) + (M.T @ M + n * np.eye(n)).T))


def to_csc(M):
    """(colptr, rowval, nzval) of the non-zeros of a dense matrix, 0-based int64."""
    cp, ri, nz = [0], [], []
    for j in range(M.shape[1]):
        rows = np.nonzero(M[:, j])[0]
        ri += rows.tolist(); nz += M[rows, j].tolist(); cp.append(len(ri))
    return np.array(cp, np.int64), np.array(ri, np.int64), np.array(nz, np.float64)


def problem(n=3, m=2, count=1):
    rng = np.random.default_rng(100 * n + m)
    A = np.asfortranarray(rng.standard_normal((max(m, 1), n)))[:m]
    return dict(n=n, m=m, P=spd(n), ldp=n, A=np.asfortranarray(A), lda=max(m, 1), q=rng.standard_normal(count * n), l=-np.ones(count * m), u=np.ones(count * m),
                dtype=0, device=0, out=True)


def dense_args(n=3, m=2):
    return problem(n, m)


def shared_args(n=3, m=2):
    return dict(problem(n, m, 2), count=2)


def batch_args(n=3, m=2):
    a = dict(problem(n, m, 2), count=2)
    a["P"] = np.concatenate([a["P"].flatten(order="F")] * 2).reshape(2, n, n)         # [count][n * n]; P symmetric, so the order of a QP's entries is moot
    a["A"] = np.concatenate([a["A"].flatten(order="F")] * 2)
    return a


def csc_fields(a, name, M):
    a[name + "cp"], a[name + "ri"], a[name + "nz"] = to_csc(M)


def csc_args(n=3, m=2, count=1):
    a = problem(n, m, count)
    P, A = a.pop("P"), a.pop("A")
    csc_fields(a, "P", P); csc_fields(a, "A", A)
    return dict(a, base=0, dense_path=0, count=count)


def csc_shared_args(n=3, m=2):
    return csc_args(n, m, 2)


def proxqp_args(n=3, me=1, mi=2):
    rng = np.random.default_rng(7)
    return dict(n=n, me=me, mi=mi, P=spd(n), ldp=n, q=rng.standard_normal(n), A=np.asfortranarray(rng.standard_normal((me, n))), lda=me, b=np.zeros(me),
                C=np.asfortranarray(rng.standard_normal((mi, n))), ldc=mi, d=np.ones(mi), dtype=0, device=0, out=True)


def proxqp_csc_args():
    a = proxqp_args()
    for k in ("P", "A", "C"):
        csc_fields(a, k, a.pop(k))
    return dict(a, base=0)


# ---------------------------------------------------------------------------------------------------------------------
# the calls
# ---------------------------------------------------------------------------------------------------------------------
def _created(rc, h):
    return rc, (h if h.value else None), None


def call_dense(L, a):
    h = C.c_void_p()
    return _created(L.qps_create_dense(a["n"], a["m"], ptr(a["P"]), a["ldp"], ptr(a["A"]), a["lda"], ptr(a["q"]), ptr(a["l"]), ptr(a["u"]), a["dtype"], a["device"],
                                       C.byref(h) if a["out"] else None), h)


def call_csc(L, a):
    h = C.c_void_p()
    return _created(L.qps_create_csc(a["n"], a["m"], ptr(a["Pcp"]), ptr(a["Pri"]), ptr(a["Pnz"]), ptr(a["Acp"]), ptr(a["Ari"]), ptr(a["Anz"]), ptr(a["q"]), ptr(a["l"]),
                                     ptr(a["u"]), a["base"], a["dense_path"], a["dtype"], a["device"], C.byref(h) if a["out"] else None), h)


def call_batch(L, a):
    h = C.c_void_p()
    return _created(L.qps_create_dense_batch(a["count"], a["n"], a["m"], ptr(a["P"]), ptr(a["A"]), ptr(a["q"]), ptr(a["l"]), ptr(a["u"]), a["dtype"], a["device"],
                                             C.byref(h) if a["out"] else None), h)


def call_shared(L, a):
    h = C.c_void_p()
    return _created(L.qps_create_dense_shared_batch(a["count"], a["n"], a["m"], ptr(a["P"]), a["ldp"], ptr(a["A"]), a["lda"], ptr(a["q"]), ptr(a["l"]), ptr(a["u"]),
                                                    a["dtype"], a["device"], C.byref(h) if a["out"] else None), h)


def call_csc_shared(L, a):
    h = C.c_void_p()
    return _created(L.qps_create_csc_shared_batch(a["count"], a["n"], a["m"], ptr(a["Pcp"]), ptr(a["Pri"]), ptr(a["Pnz"]), ptr(a["Acp"]), ptr(a["Ari"]), ptr(a["Anz"]),
                                                  ptr(a["q"]), ptr(a["l"]), ptr(a["u"]), a["base"], a["dtype"], a["device"], C.byref(h) if a["out"] else None), h)


def call_proxqp(L, a):
    h = C.c_void_p()
    return _created(L.qps_proxqp_create_dense(a["n"], a["me"], a["mi"], ptr(a["P"]), a["ldp"], ptr(a["q"]), ptr(a["A"]), a["lda"], ptr(a["b"]), ptr(a["C"]), a["ldc"],
                                              ptr(a["d"]), a["dtype"], a["device"], C.byref(h) if a["out"] else None), h)


def call_proxqp_csc(L, a):
    h = C.c_void_p()
    return _created(L.qps_proxqp_create_csc(a["n"], a["me"], a["mi"], ptr(a["Pcp"]), ptr(a["Pri"]), ptr(a["Pnz"]), ptr(a["q"]), ptr(a["Acp"]), ptr(a["Ari"]), ptr(a["Anz"]),
                                            ptr(a["b"]), ptr(a["Ccp"]), ptr(a["Cri"]), ptr(a["Cnz"]), ptr(a["d"]), a["base"], a["dtype"], a["device"],
                                            C.byref(h) if a["out"] else None), h)


# ---------------------------------------------------------------------------------------------------------------------
# faults: name -> edit of the argument dict.  `chain`: the creator's own order; `also`: further single faults that share a test with a chain member.
# ---------------------------------------------------------------------------------------------------------------------
def setk(**kw):
    return lambda a: a.update(kw)


def poke(key, idx, value):
    def f(a):
        a[key][idx] = value
    return f


def bump(key, idx):
    def f(a):
        a[key][idx] += 1
    return f


def m_zero_csc(a):
    a.update(m=0, Acp=np.zeros(a["n"] + 1, np.int64), Ari=np.zeros(0, np.int64), Anz=np.zeros(0), l=np.zeros(0), u=np.zeros(0))


def csc_faults(k, label=None):
    """The CSC walk of one matrix (fields k + cp / ri / nz) in its order: start, monotone, NULL values, row range, NaN."""
    p = label or k
    return [(f"{p}_colptr_start", bump(k + "cp", 0)), (f"{p}_colptr_not_monotone", poke(k + "cp", 2, 0)), (f"{p}_nzval_null", setk(**{k + "nz": None})),
            (f"{p}_row_out_of_range", poke(k + "ri", 1, 9)), (f"{p}_nan", poke(k + "nz", 0, np.nan))]


HEAD = [("out_null", setk(out=False)), ("bad_n", setk(n=0))]
COUNT = ("bad_count", setk(count=0))
VEC_TAIL = [("nan_q", poke("q", 0, np.nan)), ("nan_l", poke("l", 0, np.nan))]

DENSE_CHAIN = HEAD + [("too_large", setk(m=(1 << 24) + 1)), ("null_P", setk(P=None)), ("bad_ldp", setk(ldp=2)), ("bad_dtype", setk(dtype=7)),
                      ("nan_P", poke("P", (1, 1), np.nan)), ("nan_A", poke("A", (0, 1), np.nan))] + VEC_TAIL + [("asym_P", bump("P", (2, 0)))]
DENSE_ALSO = [("neg_m", setk(m=-1)), ("n_too_large", setk(n=(1 << 20) + 1)), ("null_q", setk(q=None)), ("null_A", setk(A=None)), ("null_l", setk(l=None)),
              ("null_u", setk(u=None)), ("bad_lda", setk(lda=1)), ("inf_P", poke("P", (0, 0), np.inf)), ("inf_q", poke("q", 1, np.inf)),
              ("nan_u", poke("u", 1, np.nan))]
# (what the issue names besides the adjacent pairs)
DENSE_PAIRS = [("null_P", "bad_dtype"), ("bad_ldp", "nan_P"), ("nan_q", "asym_P")]
BAD_DEVICE = ("bad_device", setk(device=-1))                              # the device check comes last: a refusal before it wins over a bad index

BATCH_CHAIN = [HEAD[0], COUNT, HEAD[1], ("null_P", setk(P=None)), ("bad_dtype", setk(dtype=7)), ("nan_P", poke("P", (1, 1, 1), np.nan)),
               ("nan_l", poke("l", 2, np.nan)), ("asym_P", bump("P", (1, 2, 0)))]
BATCH_ALSO = [("count_too_large", setk(count=65536)), ("neg_m", setk(m=-1)), ("null_q", setk(q=None)), ("null_A", setk(A=None)), ("nan_A", poke("A", 7, np.nan)),
              ("nan_q", poke("q", 4, np.nan)), ("nan_u", poke("u", 3, np.nan)), ("asym_P_first_qp", bump("P", (0, 1, 0)))]
BATCH_PAIRS = [("bad_count", "bad_n"), ("null_P", "bad_dtype")]

SHARED_CHAIN = [HEAD[0], COUNT, HEAD[1]] + DENSE_CHAIN[2:] + [("m_zero", setk(m=0))]
SHARED_ALSO = [("count_too_large", setk(count=65536)), ("nan_q_last_column", poke("q", 5, np.nan)), ("nan_u_last_column", poke("u", 3, np.nan))] + DENSE_ALSO
SHARED_PAIRS = DENSE_PAIRS + [("bad_count", "bad_n"), ("nan_q", "m_zero"), ("nan_P", "m_zero")]

CSC_MID = [("null_Pcp", setk(Pcp=None)), ("bad_index_base", setk(base=2)), ("bad_dtype", setk(dtype=7))] + csc_faults("P") + csc_faults("A") + VEC_TAIL + \
          [("asym_P", bump("Pnz", 1))]
CSC_CHAIN = HEAD + CSC_MID
CSC_ALSO = [("neg_m", setk(m=-1)), ("null_q", setk(q=None)), ("null_Acp", setk(Acp=None)), ("null_l", setk(l=None)), ("null_u", setk(u=None)),
            ("P_rowval_null", setk(Pri=None)), ("nan_u", poke("u", 1, np.nan)), ("index_base_1_with_0_based_arrays", setk(base=1))]
CSC_PAIRS = [("null_Pcp", "bad_dtype"), ("nan_q", "asym_P")]
CSC_SHARED_CHAIN = [HEAD[0], COUNT, HEAD[1], ("kkt_too_large", setk(m=1 << 27))] + CSC_MID + [("m_zero", m_zero_csc)]
CSC_SHARED_ALSO = [("count_too_large", setk(count=65536)), ("nan_q_last_column", poke("q", 5, np.nan))] + CSC_ALSO
CSC_SHARED_PAIRS = CSC_PAIRS + [("bad_count", "bad_n"), ("nan_q", "m_zero")]

PROXQP_CHAIN = [HEAD[0], ("bad_n", setk(n=0)), ("too_large", setk(mi=(1 << 20) + 1)), ("null_P", setk(P=None)), ("bad_ldp", setk(ldp=2)), ("bad_dtype", setk(dtype=7))]
PROXQP_ALSO = [("neg_me", setk(me=-1)), ("neg_mi", setk(mi=-1)), ("n_too_large", setk(n=(1 << 16) + 1)), ("null_q", setk(q=None)), ("null_A", setk(A=None)),
               ("null_b", setk(b=None)), ("null_C", setk(C=None)), ("null_d", setk(d=None)), ("bad_lda", setk(lda=0)), ("bad_ldc", setk(ldc=1))]
PROXQP_AFTER_DEVICE = [("nan_P", poke("P", (1, 1), np.nan)), ("nan_A", poke("A", (0, 1), np.nan)), ("nan_C", poke("C", (1, 0), np.nan)), ("nan_q", poke("q", 0, np.nan))]
PROXQP_CSC_CHAIN = HEAD + [("null_Pcp", setk(Pcp=None)), ("bad_index_base", setk(base=2)), ("bad_dtype", setk(dtype=7))] + csc_faults("P", "mP") + csc_faults("A", "mA") + \
                   csc_faults("C", "mC") + [("nan_q", poke("q", 0, np.nan))]
PROXQP_CSC_ALSO = [("neg_me", setk(me=-1)), ("null_q", setk(q=None)), ("null_Acp", setk(Acp=None)), ("null_b", setk(b=None)), ("null_Ccp", setk(Ccp=None)),
                   ("null_d", setk(d=None)), ("mP_rowval_null", setk(Pri=None)), ("nan_b", poke("b", 0, np.nan)), ("nan_d", poke("d", 1, np.nan))]


def _both(f, g):
    def h(a):
        f(a); g(a)
    return h


def add(name, call, args, edit=None, device=False, first=None, env=None):
    def build():
        a = args()
        if edit:
            edit(a)
        return a
    assert all(c.name != name for c in CASES), name
    CASES.append(Case(name, call, build, device, first, env or {}))


def creator_cases(fn, call, args, chain, also=(), pairs=(), last_pair=True):
    faults = dict(chain); faults.update(dict(also))
    for k, f in list(chain) + list(also):
        add(f"{fn}:{k}", call, args, f)
    adjacent = [(chain[i][0], chain[i + 1][0]) for i in range(len(chain) - 1)]
    for k1, k2 in dict.fromkeys(adjacent + list(pairs)):
        add(f"{fn}:{k1}+{k2}", call, args, _both(faults[k1], faults[k2]), first=f"{fn}:{k1}")
    if last_pair:
        add(f"{fn}:{chain[-1][0]}+bad_device", call, args, _both(chain[-1][1], BAD_DEVICE[1]), first=f"{fn}:{chain[-1][0]}")
    add(f"{fn}:well_formed", call, args, device=True)


def asym70(args, key):
    """n = 70, an entry one ulp off at (66, 3): outside the first 64 x 64 tile, as test_asymmetric_p_is_refused_like_issymmetric places it."""
    def build():
        a = args(70, 5)
        if key == "P":
            a["P"][(66, 3) if a["P"].ndim == 2 else (1, 3, 66)] = np.nextafter(a["P"][(66, 3) if a["P"].ndim == 2 else (1, 3, 66)], np.inf)
        else:
            k = int(a["Pcp"][3]) + int(np.nonzero(a["Pri"][a["Pcp"][3]:a["Pcp"][4]] == 66)[0][0])
            a["Pnz"][k] = np.nextafter(a["Pnz"][k], np.inf)
        return a
    return build


creator_cases("qps_create_dense", call_dense, dense_args, DENSE_CHAIN, DENSE_ALSO, DENSE_PAIRS)
creator_cases("qps_create_csc", call_csc, csc_args, CSC_CHAIN, CSC_ALSO, CSC_PAIRS)
creator_cases("qps_create_dense_batch", call_batch, batch_args, BATCH_CHAIN, BATCH_ALSO, BATCH_PAIRS)
creator_cases("qps_create_dense_shared_batch", call_shared, shared_args, SHARED_CHAIN, SHARED_ALSO, SHARED_PAIRS)
creator_cases("qps_create_csc_shared_batch", call_csc_shared, csc_shared_args, CSC_SHARED_CHAIN, CSC_SHARED_ALSO, CSC_SHARED_PAIRS)
creator_cases("qps_proxqp_create_dense", call_proxqp, proxqp_args, PROXQP_CHAIN, PROXQP_ALSO, last_pair=False)
creator_cases("qps_proxqp_create_csc", call_proxqp_csc, proxqp_csc_args, PROXQP_CSC_CHAIN, PROXQP_CSC_ALSO)
for _k, _f in PROXQP_AFTER_DEVICE:                                        # NO_DEVICE without a GPU, NOT_FINITE with one: see PROXQP_FINITENESS
    add(f"qps_proxqp_create_dense:{_k}", call_proxqp, proxqp_args, _f, device=True)
for _fn, _call, _args, _key in (("qps_create_dense", call_dense, dense_args, "P"), ("qps_create_dense_shared_batch", call_shared, shared_args, "P"),
                                ("qps_create_dense_batch", call_batch, batch_args, "P"), ("qps_create_csc", call_csc, csc_args, "Pnz"),
                                ("qps_create_csc_shared_batch", call_csc_shared, csc_shared_args, "Pnz")):
    CASES.append(Case(f"{_fn}:asym_P_n70_outside_first_tile", _call, asym70(_args, _key), False, None, {}))


# ---------------------------------------------------------------------------------------------------------------------
# qps_solve_batch_multi (needs no handle) and, through it, every refusal of validate_params
# ---------------------------------------------------------------------------------------------------------------------
def params(L, **kw):
    from quadraticprogramsolver_amd import _lib
    p = _lib.QpsParams()
    L.qps_default_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def multi_args():
    a = batch_args()
    a.update(devices=np.zeros(1, np.int32), workers=1, chunk=0, x=np.zeros(6), params={}, null_params=False)
    return a


def call_multi(L, a):
    p = None if a["null_params"] else C.byref(params(L, **a["params"]))
    return L.qps_solve_batch_multi(a["count"], a["n"], a["m"], ptr(a["P"]), ptr(a["A"]), ptr(a["q"]), ptr(a["l"]), ptr(a["u"]), a["dtype"], ptr(a["devices"]),
                                   a["workers"], a["chunk"], ptr(a["x"]), p, None, None, None), None, None


def par(**kw):
    return lambda a: a["params"].update(kw)


MULTI_CHAIN = [("bad_count", setk(count=0)), ("null_P", setk(P=None)), ("null_devices", setk(devices=None)), ("chunk_too_large", setk(chunk=65536)),
               ("params_null", setk(null_params=True))]
PARAM_CHAIN = [("numIterations_negative", par(numIterations=-1)), ("numItrConv_zero", par(numItrConv=0)), ("rho_zero", par(rho=0.0)), ("sigma_negative", par(sigma=-1.0)),
               ("alpha_inf", par(alpha=np.inf)), ("epsAbs_nan", par(epsAbs=np.nan)), ("fctrRho_zero", par(adptRho=1, fctrRho=0.0))]
MULTI_ALSO = [("bad_n", setk(n=0)), ("neg_m", setk(m=-1)), ("null_x", setk(x=None)), ("null_l", setk(l=None)), ("no_workers", setk(workers=0)),
              ("too_many_workers", setk(workers=257)), ("rho_inf", par(rho=np.inf)), ("rho_nan", par(rho=np.nan)), ("sigma_nan", par(sigma=np.nan)),
              ("alpha_nan", par(alpha=np.nan)), ("epsRel_nan", par(epsRel=np.nan))]
_multi = dict(MULTI_CHAIN + PARAM_CHAIN + MULTI_ALSO)
for _k, _f in MULTI_CHAIN + PARAM_CHAIN + MULTI_ALSO:
    add(f"qps_solve_batch_multi:{_k}", call_multi, multi_args, _f)
for _c in (MULTI_CHAIN[:4] + [PARAM_CHAIN[0]], [MULTI_CHAIN[3], MULTI_CHAIN[4]], PARAM_CHAIN):     # (NULL params and a bad field cannot be had together)
    for (_k1, _f1), (_k2, _f2) in zip(_c[:-1], _c[1:]):
        add(f"qps_solve_batch_multi:{_k1}+{_k2}", call_multi, multi_args, _both(_f1, _f2), first=f"qps_solve_batch_multi:{_k1}")
add("qps_solve_batch_multi:fctrRho_zero+bad_device", call_multi, multi_args, _both(_multi["fctrRho_zero"], poke("devices", 0, -1)),
    first="qps_solve_batch_multi:fctrRho_zero")


# ---------------------------------------------------------------------------------------------------------------------
# qps_ldl_analyze: every refusal, and one accepted 4 x 4 pattern with its permutation and report
# ---------------------------------------------------------------------------------------------------------------------
def ldl_args():
    P = np.array([[4.0, 1, 0, 0], [1, 4, 1, 0], [0, 1, 4, 1], [0, 0, 1, 4]])
    A = np.array([[1.0, 0, 0, 1], [0, 1, 1, 0]])
    a = dict(n=4, m=2, base=0)
    csc_fields(a, "P", P); csc_fields(a, "A", A)
    return a


def call_ldl(L, a):
    from quadraticprogramsolver_amd import _lib
    perm = np.full(max(a["n"] + a["m"], 1) if a["n"] + a["m"] < 100 else 1, -1, np.int64)
    rep = _lib.QpsLdlReport()
    rc = L.qps_ldl_analyze(a["n"], a["m"], ptr(a["Pcp"]), ptr(a["Pri"]), ptr(a["Acp"]), ptr(a["Ari"]), a["base"], ptr(perm), C.byref(rep))
    return rc, None, ({"perm": perm.tolist(), "report": rep.as_dict()} if rc == 0 else None)


def one_based(a):
    a["base"] = 1
    for k in ("Pcp", "Pri", "Acp", "Ari"):
        a[k] = a[k] + 1


LDL_CHAIN = [("bad_n", setk(n=0)), ("null_Pcp", setk(Pcp=None)), ("bad_index_base", setk(base=2)), ("P_colptr_not_monotone", poke("Pcp", 2, 1)),
             ("P_row_out_of_range", poke("Pri", 0, 4)), ("A_row_out_of_range", poke("Ari", 0, 2))]
LDL_ALSO = [("neg_m", setk(m=-1)), ("too_many_rows", setk(m=2000000000)), ("null_Acp", setk(Acp=None)), ("null_Pri", setk(Pri=None)), ("null_Ari", setk(Ari=None)),
            ("A_colptr_not_monotone", poke("Acp", 2, 0)), ("P_row_negative", poke("Pri", 0, -1))]
for _k, _f in LDL_CHAIN + LDL_ALSO:
    add(f"qps_ldl_analyze:{_k}", call_ldl, ldl_args, _f)
for (_k1, _f1), (_k2, _f2) in zip(LDL_CHAIN[:-1], LDL_CHAIN[1:]):
    add(f"qps_ldl_analyze:{_k1}+{_k2}", call_ldl, ldl_args, _both(_f1, _f2), first=f"qps_ldl_analyze:{_k1}")
add("qps_ldl_analyze:accepted_4x4", call_ldl, ldl_args)
add("qps_ldl_analyze:accepted_4x4_one_based", call_ldl, ldl_args, one_based)
# the limits come from the environment at every call: a one-column tail and one level leave this pattern too deep
add("qps_ldl_analyze:refused_by_the_level_limit", call_ldl, ldl_args, env={"QPS_LDL_MAX_TAIL": "1", "QPS_LDL_MIN_LEVEL": "1", "QPS_LDL_MAX_LEVELS": "1"})
add("qps_create_csc_shared_batch:refused_by_the_level_limit", call_csc_shared, csc_shared_args,
    env={"QPS_LDL_MAX_TAIL": "1", "QPS_LDL_MIN_LEVEL": "1", "QPS_LDL_MAX_LEVELS": "1"})
add("qps_ldl_analyze:accepted_4x4_small_tail", call_ldl, ldl_args, env={"QPS_LDL_MAX_TAIL": "2", "QPS_LDL_MIN_LEVEL": "1", "QPS_LDL_MAX_LEVELS": "64"})


# ---------------------------------------------------------------------------------------------------------------------
# every handle-taking entry point with a NULL handle (arguments otherwise well formed unless the name says so)
# ---------------------------------------------------------------------------------------------------------------------
def _null_handle_args(L):
    from quadraticprogramsolver_amd import _lib
    v = np.zeros(4)
    pp = _lib.QpsProxQpParams(); L.qps_proxqp_default_params(C.byref(pp))
    return v, ptr(v), C.byref(params(L)), C.byref(pp)


NULL_HANDLE = {   # (L, v, p, pp): a double vector, qps_params, qps_proxqp_params
    "qps_solve": lambda L, v, p, pp: L.qps_solve(None, v, p, None),
    "qps_polish": lambda L, v, p, pp: L.qps_polish(None, v, v, p, None),
    "qps_get_dual": lambda L, v, p, pp: L.qps_get_dual(None, v, v),
    "qps_linsys_init": lambda L, v, p, pp: L.qps_linsys_init(None, 1.0, 1e-6, 0, 0),
    "qps_linsys_solve": lambda L, v, p, pp: L.qps_linsys_solve(None, v, v, v, 1.0, 1e-6, 0, v, v),
    "qps_operator_apply": lambda L, v, p, pp: L.qps_operator_apply(None, 0, v, v, 0.0, 0.0),
    "qps_linsys_set_cg": lambda L, v, p, pp: L.qps_linsys_set_cg(None, 1e-6, 10),
    "qps_solve_batch": lambda L, v, p, pp: L.qps_solve_batch(None, v, p, None),
    "qps_update_shared_vectors": lambda L, v, p, pp: L.qps_update_shared_vectors(None, v, v, v),
    "qps_set_shared_rho_scale": lambda L, v, p, pp: L.qps_set_shared_rho_scale(None, v),
    "qps_set_shared_adaptive_rho": lambda L, v, p, pp: L.qps_set_shared_adaptive_rho(None, 1),
    "qps_set_shared_adaptive_rho:bad_mode": lambda L, v, p, pp: L.qps_set_shared_adaptive_rho(None, 3),
    "qps_set_shared_warm_start": lambda L, v, p, pp: L.qps_set_shared_warm_start(None, 1),
    "qps_set_shared_dual": lambda L, v, p, pp: L.qps_set_shared_dual(None, v, v),
    "qps_set_shared_infeasibility": lambda L, v, p, pp: L.qps_set_shared_infeasibility(None, 1e-4, 1e-4),
    "qps_get_shared_certificate": lambda L, v, p, pp: L.qps_get_shared_certificate(None, v, v),
    "qps_polish_shared": lambda L, v, p, pp: L.qps_polish_shared(None, v, v, p, None),
    "qps_set_shared_polish": lambda L, v, p, pp: L.qps_set_shared_polish(None, 1),
    "qps_set_shared_equilibration": lambda L, v, p, pp: L.qps_set_shared_equilibration(None, 5),
    "qps_get_shared_equilibration": lambda L, v, p, pp: L.qps_get_shared_equilibration(None, v, v),
    "qps_set_profiling": lambda L, v, p, pp: L.qps_set_profiling(None, 1),
    "qps_kernel_times": lambda L, v, p, pp: L.qps_kernel_times(None, None, 0, C.byref(C.c_int32())),
    "qps_proxqp_init_kkt": lambda L, v, p, pp: L.qps_proxqp_init_kkt(None),
    "qps_proxqp_set_state": lambda L, v, p, pp: L.qps_proxqp_set_state(None, v, v, v, v),
    "qps_proxqp_get_state": lambda L, v, p, pp: L.qps_proxqp_get_state(None, v, v, v, v),
    "qps_proxqp_solve": lambda L, v, p, pp: L.qps_proxqp_solve(None, pp, None),
    "qps_destroy": lambda L, v, p, pp: L.qps_destroy(None),
    "qps_default_params": lambda L, v, p, pp: L.qps_default_params(None),
    "qps_proxqp_default_params": lambda L, v, p, pp: L.qps_proxqp_default_params(None),
}


def _null_case(key):
    def call(L, a):
        keep, v, p, pp = _null_handle_args(L)
        prime(L)                                                          # (building the arguments called the library)
        return NULL_HANDLE[key](L, v, p, pp), None, None
    return call


for _k in NULL_HANDLE:
    add(f"null_handle:{_k}", _null_case(_k), dict)

BY_NAME = {c.name: c for c in CASES}
DEVICE_CASES = [c.name for c in CASES if c.device]


# ---------------------------------------------------------------------------------------------------------------------
# The gates that need a handle (tests/test_gpu_capi_gates.py; the fixture's "gates" section): every qps_*_shared_* entry point on the handles that are
# no shared-matrix batch, the refused arguments of a shared handle, and the entry points that want another kind of handle.
# ---------------------------------------------------------------------------------------------------------------------
def _must(rc_h):
    rc, h, _ = rc_h
    assert rc == 0 and h is not None, rc
    return h


def gate_handles(L):
    """name -> handle: dense (4, 3), CSC (4, 3), a fused dense batch 2 x (64, 64), a fallback batch 2 x (4, 0), ProxQP dense (4, 1, 2), dense shared 2 x (4, 3)."""
    return {"dense": _must(call_dense(L, dense_args(4, 3))), "csc": _must(call_csc(L, csc_args(4, 3))), "fused_batch": _must(call_batch(L, batch_args(64, 64))),
            "fallback_batch": _must(call_batch(L, batch_args(4, 0))), "proxqp": _must(call_proxqp(L, proxqp_args(4, 1, 2))),
            "shared": _must(call_shared(L, shared_args(4, 3)))}


def shared_calls(L, v, p):
    """The qps_*_shared_* entry points with well-formed arguments (v: a pointer to enough zeros / ones; p: qps_params)."""
    return {"qps_update_shared_vectors": lambda h: L.qps_update_shared_vectors(h, v, None, None), "qps_set_shared_rho_scale": lambda h: L.qps_set_shared_rho_scale(h, None),
            "qps_set_shared_adaptive_rho": lambda h: L.qps_set_shared_adaptive_rho(h, 0), "qps_set_shared_warm_start": lambda h: L.qps_set_shared_warm_start(h, 0),
            "qps_set_shared_dual": lambda h: L.qps_set_shared_dual(h, v, v), "qps_set_shared_infeasibility": lambda h: L.qps_set_shared_infeasibility(h, 0.0, 0.0),
            "qps_get_shared_certificate": lambda h: L.qps_get_shared_certificate(h, None, None), "qps_polish_shared": lambda h: L.qps_polish_shared(h, v, None, p, None),
            "qps_set_shared_polish": lambda h: L.qps_set_shared_polish(h, 0), "qps_set_shared_equilibration": lambda h: L.qps_set_shared_equilibration(h, 0),
            "qps_get_shared_equilibration": lambda h: L.qps_get_shared_equilibration(h, None, None)}


def shared_refusals(L, p):
    """name -> call(h) of every refused argument of a 2 x (4, 3) shared handle."""
    nan8, zeros8 = np.full(8, np.nan), np.zeros(8)
    scale0 = np.array([1.0, 0.0, 2.0])
    keep = (nan8, zeros8, scale0)
    nan, z, s0 = (ptr(a) for a in keep)
    return keep, {
        "qps_set_shared_adaptive_rho:mode_3": lambda h: L.qps_set_shared_adaptive_rho(h, 3),
        "qps_set_shared_warm_start:mode_3": lambda h: L.qps_set_shared_warm_start(h, 3),
        "qps_set_shared_polish:on_3": lambda h: L.qps_set_shared_polish(h, 3),
        "qps_set_shared_equilibration:passes_51": lambda h: L.qps_set_shared_equilibration(h, 51),
        "qps_set_shared_infeasibility:negative_eps": lambda h: L.qps_set_shared_infeasibility(h, -1e-4, 1e-4),
        "qps_set_shared_infeasibility:nan_eps": lambda h: L.qps_set_shared_infeasibility(h, 1e-4, float("nan")),
        "qps_set_shared_rho_scale:entry_0": lambda h: L.qps_set_shared_rho_scale(h, s0),
        "qps_set_shared_dual:nan_z": lambda h: L.qps_set_shared_dual(h, nan, z),
        "qps_set_shared_dual:nan_y": lambda h: L.qps_set_shared_dual(h, z, nan),
        "qps_polish_shared:nan_x": lambda h: L.qps_polish_shared(h, nan, None, p, None),
        "qps_polish_shared:nan_y": lambda h: L.qps_polish_shared(h, z, nan, p, None),
        "qps_polish_shared:null_p": lambda h: L.qps_polish_shared(h, z, None, None, None),
        "qps_polish_shared:null_x": lambda h: L.qps_polish_shared(h, None, None, p, None),
        "qps_update_shared_vectors:nan_q": lambda h: L.qps_update_shared_vectors(h, nan, None, None),
        "qps_update_shared_vectors:nan_l": lambda h: L.qps_update_shared_vectors(h, None, nan, None),
    }


def _answer(L, rc, h):
    return {"status": int(rc), "message": (L.qps_last_error(h) or b"").decode("utf-8", "replace")}


def run_gates(L, unchanged=None):
    """name -> {"status", "message" (qps_last_error of the handle)}.  ``unchanged``: a list that receives (name, bool) per refused argument of the shared
    handle -- a 10-iteration solve after the refusal gives bitwise the X it gave before."""
    from quadraticprogramsolver_amd import _lib
    out = {}
    H = gate_handles(L)
    try:
        zeros = np.zeros(256); v = ptr(zeros)
        pr = params(L, numIterations=10); p = C.byref(pr)
        for hn in ("dense", "csc", "fused_batch", "fallback_batch", "proxqp"):
            for fn, call in shared_calls(L, v, p).items():
                out[f"{fn}@{hn}"] = _answer(L, call(H[hn]), H[hn])

        def solve10():
            X = np.zeros(8)
            assert L.qps_solve_batch(H["shared"], ptr(X), p, None) == 0
            return X

        X0 = solve10()
        keep, calls = shared_refusals(L, p)
        for name, call in calls.items():
            out[f"{name}@shared"] = _answer(L, call(H["shared"]), H["shared"])
            if unchanged is not None:
                unchanged.append((name, solve10().tobytes() == X0.tobytes()))
        pp = _lib.QpsProxQpParams(); L.qps_proxqp_default_params(C.byref(pp))
        out["qps_solve@fused_batch"] = _answer(L, L.qps_solve(H["fused_batch"], v, p, None), H["fused_batch"])
        out["qps_solve@fallback_batch"] = _answer(L, L.qps_solve(H["fallback_batch"], v, p, None), H["fallback_batch"])
        out["qps_solve@proxqp"] = _answer(L, L.qps_solve(H["proxqp"], v, p, None), H["proxqp"])
        out["qps_solve_batch@dense"] = _answer(L, L.qps_solve_batch(H["dense"], v, p, None), H["dense"])
        out["qps_solve_batch@csc"] = _answer(L, L.qps_solve_batch(H["csc"], v, p, None), H["csc"])
        out["qps_proxqp_solve@dense"] = _answer(L, L.qps_proxqp_solve(H["dense"], C.byref(pp), None), H["dense"])
        out["qps_proxqp_solve@shared"] = _answer(L, L.qps_proxqp_solve(H["shared"], C.byref(pp), None), H["shared"])
        out["qps_operator_apply@fused_batch"] = _answer(L, L.qps_operator_apply(H["fused_batch"], 0, v, v, 0.0, 0.0), H["fused_batch"])
        out["qps_operator_apply@shared"] = _answer(L, L.qps_operator_apply(H["shared"], 0, v, v, 0.0, 0.0), H["shared"])
    finally:
        for h in H.values():
            L.qps_destroy(h)
    # qps_create_csc with dense_path: the size test comes after the device test (P = I of 70000 columns, one constraint row)
    n = 70000
    a = dict(n=n, m=1, Pcp=np.arange(n + 1, dtype=np.int64), Pri=np.arange(n, dtype=np.int64), Pnz=np.ones(n), Acp=np.minimum(np.arange(n + 1, dtype=np.int64), 1),
             Ari=np.zeros(1, np.int64), Anz=np.ones(1), q=np.zeros(n), l=-np.ones(1), u=np.ones(1), base=0, dense_path=1, dtype=0, device=0, out=True)
    prime(L)
    rc, h, _ = call_csc(L, a)
    out["qps_create_csc:too_large_to_densify"] = {"status": int(rc), "message": message(L)}
    assert h is None
    return out


# ---------------------------------------------------------------------------------------------------------------------
# running and recording
# ---------------------------------------------------------------------------------------------------------------------
def run_case(L, case):
    """{"status", "message"[, "extra"]} of one case; a handle that a well-formed call produced is destroyed."""
    old = {k: os.environ.get(k) for k in case.env}
    os.environ.update(case.env)
    try:
        a = case.args()
        prime(L)
        rc, h, extra = case.call(L, a)
        out = {"status": int(rc), "message": message(L)}
        if extra is not None:
            out["extra"] = extra
        if h is not None:
            L.qps_destroy(h)
        return out
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def _library(argv):
    from quadraticprogramsolver_amd import _lib
    if "--lib" in argv:
        _lib.LIB_PATH = os.path.abspath(argv[argv.index("--lib") + 1])
    return _lib.lib()


def main(argv):
    sys.path.insert(0, ROOT)
    L = _library(argv)
    fx = load_fixture() if os.path.exists(FIXTURE) else {}
    out = FIXTURE if "--out" not in argv else argv[argv.index("--out") + 1]
    if argv[0] == "record":
        assert L.qps_device_count() == 0, "the CPU section is recorded where no device is visible (the device cases answer QPS_ERR_NO_DEVICE there)"
        fx["cpu"] = {c.name: run_case(L, c) for c in CASES}
    elif argv[0] == "record-device":
        assert L.qps_device_count() > 0
        fx["with_device"] = {name: run_case(L, BY_NAME[name]) for name in DEVICE_CASES}
        fx["gates"] = run_gates(L)
    else:
        raise SystemExit(__doc__)
    with open(out, "w") as f:
        json.dump(fx, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out, {k: len(v) for k, v in fx.items()})


if __name__ == "__main__":
    main(sys.argv[1:])
