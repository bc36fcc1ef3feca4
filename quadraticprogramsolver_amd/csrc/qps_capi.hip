// qps_capi.hip -- the C ABI of include/qps.h and nothing else: the handle table, argument validation and problem import of every entry point.  The solvers live
// behind factories: make_dense (qps_dense.hip), make_dense_batch (qps_dense_batch.hip), the shared-matrix batches (qps_shared_dense.hip, qps_shared_csr.hip), make_sparse_solver
// (qps_sparse.hip) and ProxQP, dense and sparse (qps_proxqp.hip); the per-device resource pools are in qps_runtime.hip.
//
// An entry point tests its arguments in a fixed order and words every refusal itself; tests/test_capi_errors_cpu.py pins status, text and order.
// There is NO CPU fallback: without a HIP device every entry point fails with QPS_ERR_NO_DEVICE.
#include "ldl_symbolic.h"
#include <atomic>
#include <limits>
#include <memory>
#include <thread>

#include "batch_schedule.h"
#include "qps_batch.h"
#include "qps_internal.h"
#include "spmv_layout.h"
#include "qps_ldl.h"
#include "qps_proxqp.h"

using namespace qps;

namespace {

thread_local std::string g_last_error;

// =================================================================================================================
// handle plumbing
// =================================================================================================================
struct Handle {   // exactly one of impl / batch / fused_batch / proxqp is set
    SolverBase* impl = nullptr; std::vector<SolverBase*> batch; BatchSolverBase* fused_batch = nullptr; ProxQpBase* proxqp = nullptr; int64_t n = 0, m = 0; std::string err;
    ~Handle() { delete impl; delete fused_batch; delete proxqp; for (auto* s : batch) delete s; }
};
// what the qps_*_shared_* entry points ask of a handle: the shared-matrix family behind it, or nullptr
SharedFamilyOps* shared_family_of(Handle* h) { return h && h->fused_batch ? h->fused_batch->shared_family() : nullptr; }

int fail_with(Handle* h, int code, const std::string& msg) {
    g_last_error = msg;
    if (h) h->err = msg;
    return code;
}
bool all_finite(const double* p, int64_t count, bool allow_inf) {
    // branch-free over blocks (vectorises), an early exit between blocks; large arrays on several host threads
    std::atomic<int> bad{0};
    host_parallel(count, (int64_t)1 << 20, [&](int, int64_t b, int64_t e) {
        for (int64_t i0 = b; i0 < e && !bad.load(std::memory_order_relaxed); i0 += 4096) {
            const int64_t i1 = std::min(e, i0 + 4096);
            int flag = 0;
            if (allow_inf) { for (int64_t i = i0; i < i1; ++i) flag |= (p[i] != p[i]); }
            else { for (int64_t i = i0; i < i1; ++i) flag |= !(std::fabs(p[i]) <= 1.7976931348623157e308); }
            if (flag) bad.store(1, std::memory_order_relaxed);
        }
    });
    return bad.load() == 0;
}
// a column-major matrix (every column `rows` long, `ld` apart): contiguous storage is checked as one array
bool all_finite_matrix(const double* p, int64_t rows, int64_t cols, int64_t ld) {
    if (ld == rows) return all_finite(p, rows * cols, false);
    std::atomic<int> bad{0};
    host_parallel(cols, std::max<int64_t>(1, ((int64_t)1 << 20) / std::max<int64_t>(rows, 1)), [&](int, int64_t b, int64_t e) {
        for (int64_t j = b; j < e && !bad.load(std::memory_order_relaxed); ++j) {
            int flag = 0;
            for (int64_t i = 0; i < rows; ++i) flag |= !(std::fabs(p[i + j * ld]) <= 1.7976931348623157e308);
            if (flag) bad.store(1, std::memory_order_relaxed);
        }
    });
    return bad.load() == 0;
}
// issymmetric(mP) with tolerance 0, as SolveQuadraticProgram.m:166-168 (the MATLAB implementation raises; the CSR path reads the
// caller's CSC of P as its CSR and the dense check reads rows of P, so an asymmetric P would silently solve a different problem).
// Tiled so that both the (i, j) and the (j, i) walk stay inside a cached 64 x 64 block.  Returns -1 or the first offending column.
int64_t dense_asymmetry(const double* P, int64_t n, int64_t ldp) {
    const int64_t nb = (n + 63) / 64;
    std::atomic<int64_t> first{INT64_MAX};
    // block columns dealt cyclically over the host threads (block column b holds nb - b tiles); the smallest offending column wins, as in a serial sweep
    const int nt = (int)std::min<int64_t>(host_threads(), std::max<int64_t>(1, n * n / ((int64_t)1 << 20)));
    auto work = [&](int t) {
        for (int64_t b = t; b < nb; b += nt) {
            const int64_t j0 = b * 64;
            if (j0 >= first.load(std::memory_order_relaxed)) break;
            for (int64_t i0 = j0; i0 < n; i0 += 64) {
                const int64_t j1 = std::min(n, j0 + 64), i1 = std::min(n, i0 + 64);
                for (int64_t j = j0; j < j1; ++j)
                    for (int64_t i = std::max(i0, j + 1); i < i1; ++i)
                        if (P[i + j * ldp] != P[j + i * ldp]) { int64_t cur = first.load(); while (j < cur && !first.compare_exchange_weak(cur, j)) {} }
            }
        }
    };
    std::vector<std::thread> th;
    int started = 1;
    try { for (int t = 1; t < nt; ++t) { th.emplace_back(work, t); started = t + 1; } } catch (const std::system_error&) {}
    work(0);
    for (int t = started; t < nt; ++t) work(t);        // (thread creation refused: the caller takes those block columns)
    for (auto& x : th) x.join();
    const int64_t f = first.load();
    return f == INT64_MAX ? -1 : f;
}
// QPS_OK, or the code after fail_with (the creators validate their arguments before they ask, so that a CPU-only caller sees the same errors)
int require_device(int device, const char* out_of_range = "device index out of range") {
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess || cnt <= 0) return fail_with(nullptr, QPS_ERR_NO_DEVICE, "no HIP device visible: libqps_hip has no CPU fallback");
    if (device < 0 || device >= cnt) return fail_with(nullptr, QPS_ERR_BAD_ARGUMENT, out_of_range);
    return QPS_OK;
}

template <typename F> int guarded(Handle* h, F&& f) {
    try { f(); return QPS_OK; }
    catch (const QpsError& e) { return fail_with(h, e.code, e.msg); }
    catch (const std::bad_alloc&) { return fail_with(h, QPS_ERR_OUT_OF_MEMORY, "host allocation failed"); }
    catch (const std::exception& e) { return fail_with(h, QPS_ERR_HIP, e.what()); }
}

int validate_params(Handle* h, const qps_params* p) {
    if (!p) return fail_with(h, QPS_ERR_BAD_ARGUMENT, "params is NULL");
    if (p->numIterations < 0) return fail_with(h, QPS_ERR_BAD_ARGUMENT, "numIterations must be >= 0");
    if (p->numItrConv <= 0) return fail_with(h, QPS_ERR_BAD_ARGUMENT, "numItrConv must be positive");
    if (!(p->rho > 0) || !std::isfinite(p->rho)) return fail_with(h, QPS_ERR_BAD_ARGUMENT, "rho must be positive and finite");
    if (!(p->sigma >= 0) || !std::isfinite(p->sigma)) return fail_with(h, QPS_ERR_BAD_ARGUMENT, "sigma must be non-negative and finite");
    if (!std::isfinite(p->alpha)) return fail_with(h, QPS_ERR_BAD_ARGUMENT, "alpha must be finite");
    if (std::isnan(p->epsAbs) || std::isnan(p->epsRel)) return fail_with(h, QPS_ERR_BAD_ARGUMENT, "epsAbs/epsRel must not be NaN");
    if (p->adptRho && !(p->fctrRho > 0)) return fail_with(h, QPS_ERR_BAD_ARGUMENT, "fctrRho must be positive");
    return QPS_OK;
}

// ---- what the creators share.  Each returns QPS_OK or the code after fail_with, and tests in the order written. -------------------------------------------------
int check_out(qps_handle* out) {
    if (!out) return fail_with(nullptr, QPS_ERR_BAD_ARGUMENT, "out handle pointer is NULL");
    *out = nullptr;
    return QPS_OK;
}
int check_count(int64_t count) { return count <= 0 || count > 65535 ? fail_with(nullptr, QPS_ERR_BAD_DIMENSION, "batch count must be in 1..65535") : QPS_OK; }
int check_dims(int64_t n, int64_t m) { return n <= 0 || m < 0 ? fail_with(nullptr, QPS_ERR_BAD_DIMENSION, "need n >= 1 and m >= 0") : QPS_OK; }
int check_dtype(int dtype) { return dtype != QPS_F64 && dtype != QPS_F32 ? fail_with(nullptr, QPS_ERR_BAD_ARGUMENT, "unknown dtype") : QPS_OK; }
// q [count][n] finite, l / u [count][m] without NaN
int check_vectors(int64_t n, int64_t m, const double* q, const double* l, const double* u, int64_t count) {
    if (!all_finite(q, count * n, false)) return fail_with(nullptr, QPS_ERR_NOT_FINITE, "q contains NaN/Inf");
    if (m > 0 && (!all_finite(l, count * m, true) || !all_finite(u, count * m, true))) return fail_with(nullptr, QPS_ERR_NOT_FINITE, "l/u contain NaN");
    return QPS_OK;
}
int fail_asymmetric(int64_t column, Handle* h = nullptr) {                               // SolveQuadraticProgram.m:166-168
    char b[160]; snprintf(b, sizeof b, "The matrix mP must be a symmetric positive definite matrix (asymmetric entry in column %lld)", (long long)column);
    return fail_with(h, QPS_ERR_BAD_ARGUMENT, b);
}
// The matrix tests of a dense problem shape, shared by the creators and qps_update_shared_matrices (there a NULL matrix is kept and not tested; h: whose error text)
int check_dense_ld(int64_t n, int64_t m, const double* P, int64_t ldp, const double* A, int64_t lda, Handle* h = nullptr) {
    if ((P && ldp < n) || (A && m > 0 && lda < m)) return fail_with(h, QPS_ERR_BAD_DIMENSION, "leading dimension smaller than the row count");
    return QPS_OK;
}
int check_dense_finite(int64_t n, int64_t m, const double* P, int64_t ldp, const double* A, int64_t lda, Handle* h = nullptr) {
    if (P && !all_finite_matrix(P, n, n, ldp)) return fail_with(h, QPS_ERR_NOT_FINITE, "P contains NaN/Inf");
    if (A && m > 0 && !all_finite_matrix(A, m, n, lda)) return fail_with(h, QPS_ERR_NOT_FINITE, "A contains NaN/Inf");
    return QPS_OK;
}
int check_dense_symmetry(int64_t n, const double* P, int64_t ldp, Handle* h = nullptr) {
    const int64_t bad = P ? dense_asymmetry(P, n, ldp) : -1;
    return bad >= 0 ? fail_asymmetric(bad, h) : QPS_OK;
}
// ... and of a CSC problem shape (layout::validate_csc, layout::csc_asymmetry); a matrix whose colptr is NULL is kept and not tested
int check_csc_matrices(int64_t n, int64_t m, const int64_t* Pcp, const int64_t* Pri, const double* Pnz, const int64_t* Acp, const int64_t* Ari, const double* Anz,
                       int index_base, Handle* h = nullptr) {
    std::string why;
    int vc = Pcp ? layout::validate_csc(n, n, Pcp, Pri, Pnz, index_base, "P", &why) : 0;
    if (vc == 0 && Acp) vc = layout::validate_csc(m, n, Acp, Ari, Anz, index_base, "A", &why);
    return vc != 0 ? fail_with(h, vc, why) : QPS_OK;
}
int check_csc_symmetry(int64_t n, const int64_t* Pcp, const int64_t* Pri, const double* Pnz, int index_base, Handle* h = nullptr) {
    if (!Pcp) return QPS_OK;
    int64_t bad = -1;
    if (const int rc = guarded(h, [&] { bad = layout::csc_asymmetry(n, Pcp, Pri, Pnz, index_base); })) return rc;
    return bad >= 0 ? fail_asymmetric(bad, h) : QPS_OK;
}
// One dense problem shape: column-major P (ld ldp) and A (ld lda), `count` columns of q / l / u
int check_dense_shape(int64_t n, int64_t m, const double* P, int64_t ldp, const double* A, int64_t lda, const double* q, const double* l, const double* u, int dtype,
                      int64_t count) {
    if (const int rc = check_dims(n, m)) return rc;
    if (n > (1 << 20) || m > (1 << 24)) return fail_with(nullptr, QPS_ERR_BAD_DIMENSION, "dense problem too large");
    if (!P || !q || (m > 0 && (!A || !l || !u))) return fail_with(nullptr, QPS_ERR_BAD_ARGUMENT, "NULL problem array");
    if (const int rc = check_dense_ld(n, m, P, ldp, A, lda)) return rc;
    if (const int rc = check_dtype(dtype)) return rc;
    if (const int rc = check_dense_finite(n, m, P, ldp, A, lda)) return rc;
    if (const int rc = check_vectors(n, m, q, l, u, count)) return rc;
    return check_dense_symmetry(n, P, ldp);
}
// One CSC problem shape; colptr / rowval / nzval of both matrices by plain host code shared with the CPU tests (spmv_layout.cpp)
int check_csc_shape(int64_t n, int64_t m, const int64_t* Pcp, const int64_t* Pri, const double* Pnz, const int64_t* Acp, const int64_t* Ari, const double* Anz,
                    const double* q, const double* l, const double* u, int index_base, int dtype, int64_t count) {
    if (const int rc = check_dims(n, m)) return rc;
    if (!Pcp || !q || !Acp || (m > 0 && (!l || !u))) return fail_with(nullptr, QPS_ERR_BAD_ARGUMENT, "NULL problem array");
    if (index_base != 0 && index_base != 1) return fail_with(nullptr, QPS_ERR_BAD_ARGUMENT, "index_base must be 0 or 1");
    if (const int rc = check_dtype(dtype)) return rc;
    if (const int rc = check_csc_matrices(n, m, Pcp, Pri, Pnz, Acp, Ari, Anz, index_base)) return rc;
    if (const int rc = check_vectors(n, m, q, l, u, count)) return rc;
    return check_csc_symmetry(n, Pcp, Pri, Pnz, index_base);
}
// CSC (rows x n) -> column-major dense with leading dimension max(rows, 1), duplicates summed; rows == 0: colptr is not read
std::vector<double> densify_csc(const int64_t* cp, const int64_t* ri, const double* nz, int64_t rows, int64_t n, int index_base) {
    std::vector<double> D((size_t)std::max<int64_t>(rows, 1) * n, 0.0);
    for (int64_t j = 0; rows > 0 && j < n; ++j)
        for (int64_t k = cp[j] - index_base; k < cp[j + 1] - index_base; ++k) D[(size_t)(ri[k] - index_base) + (size_t)j * rows] += nz[k];
    return D;
}
// The end of every creator: the device, a Handle, `build(handle)` under guarded (a failed build leaves no handle), *out
template <typename F> int create_handle(int device, int64_t n, int64_t m, qps_handle* out, F&& build) {
    if (const int dc = require_device(device)) return dc;
    auto h = std::make_unique<Handle>(); h->n = n; h->m = m;
    if (const int rc = guarded(nullptr, [&] { build(*h); })) return rc;
    *out = reinterpret_cast<qps_handle>(h.release());
    return QPS_OK;
}
// The family behind a qps_*_shared_* call, or nullptr with *rc = QPS_ERR_UNSUPPORTED after fail_with; `takes` closes the sentence about these handles
SharedFamilyOps* shared_gate(Handle* h, const char* fn, const char* takes, int* rc) {
    SharedFamilyOps* fam = shared_family_of(h);
    if (!fam) *rc = fail_with(h, QPS_ERR_UNSUPPORTED, std::string(fn) + ": only shared-matrix batch handles (qps_create_dense_shared_batch, qps_create_csc_shared_batch) " + takes);
    return fam;
}

}  // namespace

extern "C" {

#define QPS_API __attribute__((visibility("default")))

QPS_API int32_t qps_default_params(qps_params* p) {
    if (!p) return QPS_ERR_BAD_ARGUMENT;
    memset(p, 0, sizeof(*p));
    p->numIterations = 5000; p->epsAbs = 1e-6; p->epsRel = 1e-6;            // SolveQuadraticProgram.jl:15
    p->rho = 1.0; p->sigma = 1e-6; p->alpha = 1.6; p->delta = 1e-6; p->adptRho = 0;   // :16
    p->fctrRho = 5.0; p->numItrConv = 25; p->numItrPolish = 10; p->epsMinres = 1e-6; p->numItrMinres = 500;   // :17
    p->linsys = QPS_LINSYS_AUTO; p->trsvBlock = 0; p->reuseFactor = 0; p->loopVariant = 0;
    p->epsPcg = 1e-6; p->numItrPcg = 1000;                                  // LinearSystemSolvers.jl:125
    return QPS_OK;
}

QPS_API int32_t qps_device_count(void) {
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess) return 0;
    return cnt;
}

QPS_API int32_t qps_create_dense(int64_t n, int64_t m, const double* P, int64_t ldp, const double* A, int64_t lda,
                                 const double* q, const double* l, const double* u, int32_t dtype, int32_t device,
                                 qps_handle* out) {
    if (const int rc = check_out(out)) return rc;
    if (const int rc = check_dense_shape(n, m, P, ldp, A, lda, q, l, u, dtype, 1)) return rc;
    return create_handle(device, n, m, out, [&](Handle& h) { h.impl = make_dense(device, n, m, dtype, P, ldp, A, lda, q, l, u); });
}

QPS_API int32_t qps_create_csc(int64_t n, int64_t m, const int64_t* Pcp, const int64_t* Pri, const double* Pnz,
                               const int64_t* Acp, const int64_t* Ari, const double* Anz, const double* q, const double* l,
                               const double* u, int32_t index_base, int32_t dense_path, int32_t dtype, int32_t device,
                               qps_handle* out) {
    if (const int rc = check_out(out)) return rc;
    if (const int rc = check_csc_shape(n, m, Pcp, Pri, Pnz, Acp, Ari, Anz, q, l, u, index_base, dtype, 1)) return rc;
    return create_handle(device, n, m, out, [&](Handle& h) {
        if (!dense_path) { h.impl = make_sparse_solver(device, n, m, dtype, Pcp, Pri, Pnz, Acp, Ari, Anz, q, l, u, index_base); return; }
        if ((double)n * n > 4e9 || (double)m * n > 8e9) throw QpsError(QPS_ERR_BAD_DIMENSION, "problem too large to densify");
        const std::vector<double> Pd = densify_csc(Pcp, Pri, Pnz, n, n, index_base), Ad = densify_csc(Acp, Ari, Anz, m, n, index_base);
        h.impl = make_dense(device, n, m, dtype, Pd.data(), n, Ad.data(), std::max<int64_t>(m, 1), q, l, u);
    });
}

QPS_API int32_t qps_solve(qps_handle hh, double* x, const qps_params* p, qps_info* info) {
    Handle* h = reinterpret_cast<Handle*>(hh);
    if (!h || !h->impl) return fail_with(h, QPS_ERR_BAD_ARGUMENT, "invalid handle");
    if (!x) return fail_with(h, QPS_ERR_BAD_ARGUMENT, "x_inout is NULL");
    int rc = validate_params(h, p);
    if (rc != QPS_OK) return rc;
    if (!all_finite(x, h->n, false)) return fail_with(h, QPS_ERR_NOT_FINITE, "x_inout (warm start) contains NaN/Inf");
    return guarded(h, [&] { h->impl->solve(x, *p, info); });
}

QPS_API int32_t qps_polish(qps_handle hh, double* x, const double* y, const qps_params* p, qps_polish_report* rep) {
    Handle* h = reinterpret_cast<Handle*>(hh);
    if (!h || !h->impl) return fail_with(h, QPS_ERR_BAD_ARGUMENT, "invalid handle");
    if (!x || (h->m > 0 && !y)) return fail_with(h, QPS_ERR_BAD_ARGUMENT, "NULL vector");
    int rc = validate_params(h, p);
    if (rc != QPS_OK) return rc;
    if (!all_finite(x, h->n, false) || !all_finite(y, h->m, false)) return fail_with(h, QPS_ERR_NOT_FINITE, "x or y contains NaN/Inf");
    return guarded(h, [&] { h->impl->polish(x, y, *p, rep); });
}

QPS_API int32_t qps_get_dual(qps_handle hh, double* z, double* y) {
    Handle* h = reinterpret_cast<Handle*>(hh);
    if (!h || (!h->impl && !h->fused_batch && h->batch.empty())) return fail_with(h, QPS_ERR_BAD_ARGUMENT, "invalid handle");
    if (h->fused_batch) return guarded(h, [&] { h->fused_batch->get_dual(z, y); });
    if (!h->impl)       // a batch of independent solvers: [count][m] like the fused batch
        return guarded(h, [&] { for (size_t b = 0; b < h->batch.size(); ++b) h->batch[b]->get_dual(z ? z + (int64_t)b * h->m : nullptr, y ? y + (int64_t)b * h->m : nullptr); });
    return guarded(h, [&] { h->impl->get_dual(z, y); });
}

QPS_API int32_t qps_linsys_init(qps_handle hh, double rho, double sigma, int32_t linsys, int32_t trsvBlock) {
    Handle* h = reinterpret_cast<Handle*>(hh);
    if (!h || !h->impl) return fail_with(h, QPS_ERR_BAD_ARGUMENT, "invalid handle");
    if (!(rho > 0) || !(sigma >= 0)) return fail_with(h, QPS_ERR_BAD_ARGUMENT, "rho must be positive, sigma non-negative");
    return guarded(h, [&] { h->impl->linsys_init(rho, sigma, linsys, trsvBlock); });
}

QPS_API int32_t qps_linsys_solve(qps_handle hh, const double* x, const double* z, const double* y, double rho, double sigma,
                                 int32_t changed, double* xx, double* zz) {
    Handle* h = reinterpret_cast<Handle*>(hh);
    if (!h || !h->impl) return fail_with(h, QPS_ERR_BAD_ARGUMENT, "invalid handle");
    if (!x || !xx || (h->m > 0 && (!z || !y || !zz))) return fail_with(h, QPS_ERR_BAD_ARGUMENT, "NULL vector");
    if (!(rho > 0) || !(sigma >= 0)) return fail_with(h, QPS_ERR_BAD_ARGUMENT, "rho must be positive, sigma non-negative");
    return guarded(h, [&] { h->impl->linsys_solve(x, z, y, rho, sigma, changed, xx, zz); });
}

QPS_API int32_t qps_operator_apply(qps_handle hh, int32_t op, const double* in, double* out, double rho, double sigma) {
    Handle* h = reinterpret_cast<Handle*>(hh);
    if (!h || !h->impl) return fail_with(h, QPS_ERR_BAD_ARGUMENT, "invalid handle (qps_operator_apply takes a single-problem handle)");
    if (op < QPS_OP_P || op > QPS_OP_REDUCED) return fail_with(h, QPS_ERR_BAD_ARGUMENT, "unknown qps_operator_kind");
    if (!in || !out) return fail_with(h, QPS_ERR_BAD_ARGUMENT, "NULL vector");
    if (op == QPS_OP_REDUCED && (!(rho >= 0) || !(sigma >= 0))) return fail_with(h, QPS_ERR_BAD_ARGUMENT, "rho and sigma must be non-negative");
    if (!all_finite(in, op == QPS_OP_AT ? h->m : h->n, false)) return fail_with(h, QPS_ERR_NOT_FINITE, "the input vector contains NaN/Inf");
    return guarded(h, [&] { h->impl->operator_apply(op, in, out, rho, sigma); });
}

QPS_API int32_t qps_linsys_set_cg(qps_handle hh, double epsPcg, int32_t numItrPcg) {
    Handle* h = reinterpret_cast<Handle*>(hh);
    if (!h || !h->impl) return fail_with(h, QPS_ERR_BAD_ARGUMENT, "invalid handle");
    if (std::isnan(epsPcg) || epsPcg < 0 || numItrPcg < 0) return fail_with(h, QPS_ERR_BAD_ARGUMENT, "need epsPcg >= 0 and numItrPcg >= 0");
    return guarded(h, [&] { h->impl->linsys_set_cg(epsPcg, numItrPcg); });
}

QPS_API int32_t qps_create_dense_batch(int64_t count, int64_t n, int64_t m, const double* P, const double* A, const double* q,
                                       const double* l, const double* u, int32_t dtype, int32_t device, qps_handle* out) {
    if (const int rc = check_out(out)) return rc;
    if (const int rc = check_count(count)) return rc;
    if (const int rc = check_dims(n, m)) return rc;
    if (!P || !q || (m > 0 && (!A || !l || !u))) return fail_with(nullptr, QPS_ERR_BAD_ARGUMENT, "NULL problem array");
    if (const int rc = check_dtype(dtype)) return rc;
    if (!all_finite(P, count * n * n, false) || !all_finite(q, count * n, false) || (m > 0 && !all_finite(A, count * m * n, false)))
        return fail_with(nullptr, QPS_ERR_NOT_FINITE, "P/A/q contain NaN/Inf");
    if (m > 0 && (!all_finite(l, count * m, true) || !all_finite(u, count * m, true))) return fail_with(nullptr, QPS_ERR_NOT_FINITE, "l/u contain NaN");
    {   // issymmetric(mP) for every QP of the batch, the QPs dealt to the host threads (64 QPs of n = 1024 took 130 ms one after the other); the first offender is reported
        std::atomic<int64_t> first_bad{INT64_MAX};
        host_parallel(count, std::max<int64_t>(1, ((int64_t)1 << 20) / (n * n)), [&](int, int64_t b0, int64_t b1) {
            for (int64_t b = b0; b < b1 && b < first_bad.load(std::memory_order_relaxed); ++b)
                if (dense_asymmetry(P + b * n * n, n, n) >= 0) { int64_t cur = first_bad.load(); while (b < cur && !first_bad.compare_exchange_weak(cur, b)) {} }
        });
        const int64_t b = first_bad.load();
        if (b != INT64_MAX) { char bf[160]; snprintf(bf, sizeof bf, "QP %lld of the batch: the matrix mP must be a symmetric positive definite matrix", (long long)b); return fail_with(nullptr, QPS_ERR_BAD_ARGUMENT, bf); }
    }
    return create_handle(device, n, m, out, [&](Handle& h) {
        h.fused_batch = make_dense_batch(device, dtype, (int)count, n, m, P, A, q, l, u);
        for (int64_t b = 0; !h.fused_batch && b < count; ++b) {   // shapes the fused pass does not cover: independent solvers, each through the single creator's checks
            const double *Ab = A ? A + b * m * n : nullptr, *lb = l ? l + b * m : nullptr, *ub = u ? u + b * m : nullptr;
            if (const int rc = check_dense_shape(n, m, P + b * n * n, n, Ab, m, q + b * n, lb, ub, dtype, 1)) throw QpsError(rc, g_last_error);
            h.batch.push_back(make_dense(device, n, m, dtype, P + b * n * n, n, Ab, m, q + b * n, lb, ub));
        }
    });
}

QPS_API int32_t qps_solve_batch(qps_handle hh, double* x, const qps_params* p, qps_info* infos) {
    Handle* h = reinterpret_cast<Handle*>(hh);
    if (!h || (h->batch.empty() && !h->fused_batch)) return fail_with(h, QPS_ERR_BAD_ARGUMENT, "not a batch handle");
    if (!x) return fail_with(h, QPS_ERR_BAD_ARGUMENT, "x_inout is NULL");
    int rc = validate_params(h, p);
    if (rc != QPS_OK) return rc;
    if (h->fused_batch) return guarded(h, [&] { h->fused_batch->solve_batch(x, *p, infos); });
    for (size_t b = 0; b < h->batch.size(); ++b) {
        rc = guarded(h, [&] { h->batch[b]->solve(x + (int64_t)b * h->n, *p, infos ? infos + b : nullptr); });
        if (rc != QPS_OK) return rc;
    }
    return QPS_OK;
}

QPS_API int32_t qps_create_dense_shared_batch(int64_t count, int64_t n, int64_t m, const double* P, int64_t ldp, const double* A, int64_t lda,
                                              const double* q, const double* l, const double* u, int32_t dtype, int32_t device, qps_handle* out) {
    if (const int rc = check_out(out)) return rc;
    if (const int rc = check_count(count)) return rc;
    if (const int rc = check_dense_shape(n, m, P, ldp, A, lda, q, l, u, dtype, count)) return rc;
    if (m == 0) return fail_with(nullptr, QPS_ERR_UNSUPPORTED, "shared-matrix batch needs m >= 1 (without constraints the columns are independent linear solves)");
    if (roundup(n, 64) > shared_batch_max_np(dtype))
        return fail_with(nullptr, QPS_ERR_UNSUPPORTED, "shared-matrix batch: n beyond the limit of the whole-factor explicit inverse (16384 fp64, 32768 fp32)");
    return create_handle(device, n, m, out, [&](Handle& h) { h.fused_batch = make_dense_shared_batch(device, dtype, (int)count, n, m, P, ldp, A, lda, q, l, u); });
}

QPS_API int32_t qps_create_csc_shared_batch(int64_t count, int64_t n, int64_t m, const int64_t* Pcp, const int64_t* Pri, const double* Pnz, const int64_t* Acp,
                                            const int64_t* Ari, const double* Anz, const double* q, const double* l, const double* u, int32_t index_base,
                                            int32_t dtype, int32_t device, qps_handle* out) {
    if (const int rc = check_out(out)) return rc;
    if (const int rc = check_count(count)) return rc;
    if (const int rc = check_dims(n, m)) return rc;                                    // (ahead of the panel limit; check_csc_shape asks again)
    if (n + m > ((int64_t)1 << 27) - 64) return fail_with(nullptr, QPS_ERR_BAD_DIMENSION, "KKT matrix too large for the panel form of the sparse direct plugin (n + m < 2^27)");
    if (const int rc = check_csc_shape(n, m, Pcp, Pri, Pnz, Acp, Ari, Anz, q, l, u, index_base, dtype, count)) return rc;
    if (m == 0) return fail_with(nullptr, QPS_ERR_UNSUPPORTED, "shared-matrix batch needs m >= 1 (without constraints the columns are independent linear solves)");
    if (Pcp[n] - index_base > 2000000000LL || Acp[n] - index_base > 2000000000LL) return fail_with(nullptr, QPS_ERR_BAD_DIMENSION, "more than 2^31 non-zeros");
    // ordering + symbolic factor: host only, once per family; the limits are read here, as SparseSolver::ldl_prepare reads them (part of the handle's layout)
    SparseSharedInput in;
    const int rc = guarded(nullptr, [&] {
        layout::canonical_csc(n, Pcp, Pri, Pnz, index_base, in.Pcp, in.Pri, in.Pnz);
        layout::canonical_csc(n, Acp, Ari, Anz, index_base, in.Acp, in.Ari, in.Anz);
        const char* e4 = getenv("QPS_LDL_PANEL_SPR");
        in.spr = e4 ? atoi(e4) : 0;   // 1 | 4 | 16: that strip count for every level of this handle; anything else: automatic
        const LdlLimits lim = ldl_limits_from_env();
        try { in.sym = ldl_analyze((int)n, (int)m, in.Pcp.data(), in.Pri.data(), in.Acp.data(), in.Ari.data(), 0, lim.max_tail, lim.min_level_width, lim.max_levels); }
        catch (const std::runtime_error& e) { throw QpsError(QPS_ERR_UNSUPPORTED, e.what()); }
    });
    if (rc != QPS_OK) return rc;
    return create_handle(device, n, m, out, [&](Handle& h) { h.fused_batch = make_sparse_shared_batch(device, dtype, (int)count, n, m, std::move(in), q, l, u); });
}

QPS_API int32_t qps_create_csc_shared_batch_cg(int64_t count, int64_t n, int64_t m, const int64_t* Pcp, const int64_t* Pri, const double* Pnz, const int64_t* Acp,
                                               const int64_t* Ari, const double* Anz, const double* q, const double* l, const double* u, int32_t index_base,
                                               int32_t dtype, int32_t device, qps_handle* out) {
    if (const int rc = check_out(out)) return rc;
    if (const int rc = check_count(count)) return rc;
    if (const int rc = check_dims(n, m)) return rc;                                    // (ahead of the panel limit; check_csc_shape asks again)
    if (n > ((int64_t)1 << 31) - 64 || m > ((int64_t)1 << 31) - 64)
        return fail_with(nullptr, QPS_ERR_BAD_DIMENSION, "problem too large for the panel form of the matrix-free CG plugin (n, m <= 2^31 - 64)");
    if (const int rc = check_csc_shape(n, m, Pcp, Pri, Pnz, Acp, Ari, Anz, q, l, u, index_base, dtype, count)) return rc;
    if (m == 0) return fail_with(nullptr, QPS_ERR_UNSUPPORTED, "shared-matrix batch needs m >= 1 (without constraints the columns are independent linear solves)");
    if (Pcp[n] - index_base > 2000000000LL || Acp[n] - index_base > 2000000000LL) return fail_with(nullptr, QPS_ERR_BAD_DIMENSION, "more than 2^31 non-zeros");
    CgSharedInput in;                                                                  // no analysis: the canonical arrays are all the host prepares
    const int rc = guarded(nullptr, [&] {
        layout::canonical_csc(n, Pcp, Pri, Pnz, index_base, in.Pcp, in.Pri, in.Pnz);
        layout::canonical_csc(n, Acp, Ari, Anz, index_base, in.Acp, in.Ari, in.Anz);
    });
    if (rc != QPS_OK) return rc;
    return create_handle(device, n, m, out, [&](Handle& h) { h.fused_batch = make_cg_shared_batch(device, dtype, (int)count, n, m, std::move(in), q, l, u); });
}

QPS_API int32_t qps_update_shared_vectors(qps_handle hh, const double* q, const double* l, const double* u) {
    Handle* h = reinterpret_cast<Handle*>(hh);
    const char* other = "not a shared-matrix batch handle";   // BAD_ARGUMENT here, not the gate's UNSUPPORTED; a fused batch of another kind has its arrays tested first
    if (!h || !h->fused_batch) return fail_with(h, QPS_ERR_BAD_ARGUMENT, other);
    const int64_t c = h->fused_batch->count;
    if (q && !all_finite(q, c * h->n, false)) return fail_with(h, QPS_ERR_NOT_FINITE, "q contains NaN/Inf");
    if ((l && !all_finite(l, c * h->m, true)) || (u && !all_finite(u, c * h->m, true))) return fail_with(h, QPS_ERR_NOT_FINITE, "l/u contain NaN");
    SharedFamilyOps* fam = shared_family_of(h);
    if (!fam) return fail_with(h, QPS_ERR_BAD_ARGUMENT, other);
    return guarded(h, [&] { fam->update_vectors(q, l, u); });
}

QPS_API int32_t qps_update_shared_matrices(qps_handle hh, const double* P, int64_t ldp, const double* A, int64_t lda) {
    Handle* h = reinterpret_cast<Handle*>(hh);
    if (!h) return fail_with(nullptr, QPS_ERR_BAD_ARGUMENT, "handle is NULL");
    int rc; SharedFamilyOps* fam = shared_gate(h, "qps_update_shared_matrices", "take new matrices on the analysis they keep", &rc);
    if (!fam) return rc;
    if (fam->takes_csc()) return guarded(h, [&] { fam->update_matrices(nullptr, 0, nullptr, 0); });   // the path words its own refusal
    if (const int c = check_dense_ld(h->n, h->m, P, ldp, A, lda, h)) return c;
    if (const int c = check_dense_finite(h->n, h->m, P, ldp, A, lda, h)) return c;
    if (const int c = check_dense_symmetry(h->n, P, ldp, h)) return c;
    return guarded(h, [&] { fam->update_matrices(P, ldp, A, lda); });
}

QPS_API int32_t qps_update_shared_matrices_csc(qps_handle hh, const int64_t* Pcp, const int64_t* Pri, const double* Pnz, const int64_t* Acp, const int64_t* Ari,
                                               const double* Anz, int32_t index_base) {
    Handle* h = reinterpret_cast<Handle*>(hh);
    if (!h) return fail_with(nullptr, QPS_ERR_BAD_ARGUMENT, "handle is NULL");
    int rc; SharedFamilyOps* fam = shared_gate(h, "qps_update_shared_matrices_csc", "take new matrices on the analysis they keep", &rc);
    if (!fam) return rc;
    CanonicalCsc Pc, Ac;
    if (!fam->takes_csc()) return guarded(h, [&] { fam->update_matrices_csc(Pc, Ac); });              // the path words its own refusal
    const bool anyP = Pcp || Pri || Pnz, anyA = Acp || Ari || Anz;
    if ((anyP && !(Pcp && Pri && Pnz)) || (anyA && !(Acp && Ari && Anz)))
        return fail_with(h, QPS_ERR_BAD_ARGUMENT, std::string("qps_update_shared_matrices_csc: colptr, rowval and nzval of ") + (anyP && !(Pcp && Pri && Pnz) ? "P" : "A") +
                                                      " must be all NULL (the matrix is kept) or all given");
    if (index_base != 0 && index_base != 1) return fail_with(h, QPS_ERR_BAD_ARGUMENT, "index_base must be 0 or 1");
    if (const int c = check_csc_matrices(h->n, h->m, Pcp, Pri, Pnz, Acp, Ari, Anz, index_base, h)) return c;
    if (const int c = check_csc_symmetry(h->n, Pcp, Pri, Pnz, index_base, h)) return c;
    return guarded(h, [&] {
        if (anyP) { layout::canonical_csc(h->n, Pcp, Pri, Pnz, index_base, Pc.cp, Pc.ri, Pc.nz); Pc.given = true; }
        if (anyA) { layout::canonical_csc(h->n, Acp, Ari, Anz, index_base, Ac.cp, Ac.ri, Ac.nz); Ac.given = true; }
        fam->update_matrices_csc(Pc, Ac);
    });
}

QPS_API int32_t qps_get_shared_pattern(qps_handle hh, int64_t* nnzP, int64_t* nnzA, int64_t* Pcp, int64_t* Pri, int64_t* Acp, int64_t* Ari) {
    Handle* h = reinterpret_cast<Handle*>(hh);
    if (!h) return fail_with(nullptr, QPS_ERR_BAD_ARGUMENT, "handle is NULL");
    int rc; SharedFamilyOps* fam = shared_gate(h, "qps_get_shared_pattern", "keep the canonical pattern they were created on", &rc);
    if (!fam) return rc;
    return guarded(h, [&] { fam->get_pattern(nnzP, nnzA, Pcp, Pri, Acp, Ari); });                     // the dense path words its own refusal
}

QPS_API int32_t qps_update_shared_values(qps_handle hh, const double* Pnz, int64_t nnzP, const double* Anz, int64_t nnzA, int32_t location) {
    Handle* h = reinterpret_cast<Handle*>(hh);
    if (!h) return fail_with(nullptr, QPS_ERR_BAD_ARGUMENT, "handle is NULL");
    int rc; SharedFamilyOps* fam = shared_gate(h, "qps_update_shared_values", "take new values on the pattern they keep", &rc);
    if (!fam) return rc;
    if (fam->takes_csc() && location != QPS_MEM_HOST && location != QPS_MEM_DEVICE)
        return fail_with(h, QPS_ERR_BAD_ARGUMENT, "qps_update_shared_values: location must be QPS_MEM_HOST (0) or QPS_MEM_DEVICE (1)");
    ValuesVerdict v;
    if (const int c = guarded(h, [&] { v = fam->update_values(Pnz, nnzP, Anz, nnzA, location); })) return c;   // (the dense path words its own refusal)
    // what the device found is worded by the host code of qps_update_shared_matrices_csc: the same values, the same code and text from both entry points
    if (v.not_finite) {
        static const int64_t cp1[2] = {0, 1}, ri1[1] = {0};
        const double nan1[1] = {std::numeric_limits<double>::quiet_NaN()};
        const bool isA = v.not_finite[0] == 'A';                                                      // validate_csc's code and text for that matrix
        return check_csc_matrices(1, 1, isA ? nullptr : cp1, ri1, nan1, isA ? cp1 : nullptr, ri1, nan1, 0, h);
    }
    if (v.asymmetric_column >= 0) return fail_asymmetric(v.asymmetric_column, h);
    return QPS_OK;
}

QPS_API int32_t qps_set_shared_rho_scale(qps_handle hh, const double* scale) {
    Handle* h = reinterpret_cast<Handle*>(hh);
    if (!h) return fail_with(nullptr, QPS_ERR_BAD_ARGUMENT, "handle is NULL");
    int rc; SharedFamilyOps* fam = shared_gate(h, "qps_set_shared_rho_scale", "take a per-row rho scale", &rc);
    if (!fam) return rc;
    for (int64_t i = 0; scale && i < h->m; ++i)
        if (!(scale[i] > 0) || !std::isfinite(scale[i])) {
            char b[128]; snprintf(b, sizeof b, "rho scale: entry %lld is not a finite positive number", (long long)i);
            return fail_with(h, QPS_ERR_BAD_ARGUMENT, b);
        }
    return guarded(h, [&] { fam->set_rho_scale(scale); });
}

QPS_API int32_t qps_set_shared_adaptive_rho(qps_handle hh, int32_t mode) {
    Handle* h = reinterpret_cast<Handle*>(hh);
    if (!h) return fail_with(nullptr, QPS_ERR_BAD_ARGUMENT, "handle is NULL");
    if (mode != 0 && mode != 1) return fail_with(h, QPS_ERR_BAD_ARGUMENT, "qps_set_shared_adaptive_rho: mode must be 0 (fixed rho) or 1 (family-wide adaptive rho)");
    int rc; SharedFamilyOps* fam = shared_gate(h, "qps_set_shared_adaptive_rho", "run the family-wide rho rule", &rc);
    if (!fam) return rc;
    if (mode && fam->column_rho)
        return fail_with(h, QPS_ERR_UNSUPPORTED, "qps_set_shared_adaptive_rho: the per-column rule is on (turn qps_set_shared_column_rho off first); the handle is unchanged");
    fam->family_rho = mode;
    return QPS_OK;
}

QPS_API int32_t qps_set_shared_column_rho(qps_handle hh, int32_t on) {
    Handle* h = reinterpret_cast<Handle*>(hh);
    if (!h) return fail_with(nullptr, QPS_ERR_BAD_ARGUMENT, "handle is NULL");
    if (on != 0 && on != 1) return fail_with(h, QPS_ERR_BAD_ARGUMENT, "qps_set_shared_column_rho: on must be 0 (off) or 1 (every column moves its own rho)");
    int rc; SharedFamilyOps* fam = shared_gate(h, "qps_set_shared_column_rho", "run the per-column rho rule", &rc);
    if (!fam) return rc;
    if (on && !fam->takes_column_rho())
        return fail_with(h, QPS_ERR_UNSUPPORTED, "qps_set_shared_column_rho: one factor serves every column of a dense or sparse L D L' shared-matrix batch, so its columns "
                                                 "cannot move rho one by one (qps_set_shared_adaptive_rho moves it for the family); only a matrix-free CG shared-matrix "
                                                 "batch takes the per-column rule");
    if (on && fam->family_rho)
        return fail_with(h, QPS_ERR_UNSUPPORTED, "qps_set_shared_column_rho: the family-wide rule is on (turn qps_set_shared_adaptive_rho off first); the handle is unchanged");
    fam->column_rho = on;
    return QPS_OK;
}

QPS_API int32_t qps_set_shared_warm_start(qps_handle hh, int32_t mode) {
    Handle* h = reinterpret_cast<Handle*>(hh);
    if (!h) return fail_with(nullptr, QPS_ERR_BAD_ARGUMENT, "handle is NULL");
    if (mode < 0 || mode > 2) return fail_with(h, QPS_ERR_BAD_ARGUMENT, "qps_set_shared_warm_start: mode must be 0 (z = y = 0), 1 (the stored z and y) or 2 (z = A x, the stored y)");
    int rc; SharedFamilyOps* fam = shared_gate(h, "qps_set_shared_warm_start", "keep z and y between solves", &rc);
    if (!fam) return rc;
    fam->warm_start = mode;
    return QPS_OK;
}

QPS_API int32_t qps_set_shared_dual(qps_handle hh, const double* z, const double* y) {
    Handle* h = reinterpret_cast<Handle*>(hh);
    if (!h) return fail_with(nullptr, QPS_ERR_BAD_ARGUMENT, "handle is NULL");
    int rc; SharedFamilyOps* fam = shared_gate(h, "qps_set_shared_dual", "keep z and y between solves", &rc);
    if (!fam) return rc;
    const int64_t c = h->fused_batch->count;
    if (z && !all_finite(z, c * h->m, false)) return fail_with(h, QPS_ERR_BAD_ARGUMENT, "qps_set_shared_dual: z contains NaN/Inf (the handle keeps its state)");
    if (y && !all_finite(y, c * h->m, false)) return fail_with(h, QPS_ERR_BAD_ARGUMENT, "qps_set_shared_dual: y contains NaN/Inf (the handle keeps its state)");
    return guarded(h, [&] { fam->set_dual(z, y); });
}

QPS_API int32_t qps_set_shared_infeasibility(qps_handle hh, double epsPrimInf, double epsDualInf) {
    Handle* h = reinterpret_cast<Handle*>(hh);
    if (!h) return fail_with(nullptr, QPS_ERR_BAD_ARGUMENT, "handle is NULL");
    if (!(epsPrimInf >= 0) || !std::isfinite(epsPrimInf) || !(epsDualInf >= 0) || !std::isfinite(epsDualInf))
        return fail_with(h, QPS_ERR_BAD_ARGUMENT, "qps_set_shared_infeasibility: epsPrimInf and epsDualInf must be finite and >= 0 (0 leaves that test off; the handle keeps its setting)");
    int rc; SharedFamilyOps* fam = shared_gate(h, "qps_set_shared_infeasibility", "issue per-column infeasibility certificates", &rc);
    if (!fam) return rc;
    return guarded(h, [&] { fam->set_infeasibility(epsPrimInf, epsDualInf); });
}

QPS_API int32_t qps_get_shared_certificate(qps_handle hh, double* dy, double* dx) {
    Handle* h = reinterpret_cast<Handle*>(hh);
    if (!h) return fail_with(nullptr, QPS_ERR_BAD_ARGUMENT, "handle is NULL");
    int rc; SharedFamilyOps* fam = shared_gate(h, "qps_get_shared_certificate", "issue per-column infeasibility certificates", &rc);
    if (!fam) return rc;
    return guarded(h, [&] { fam->get_certificate(dy, dx); });
}

QPS_API int32_t qps_polish_shared(qps_handle hh, double* x, const double* y, const qps_params* p, qps_polish_report* reports) {
    Handle* h = reinterpret_cast<Handle*>(hh);
    if (!h) return fail_with(nullptr, QPS_ERR_BAD_ARGUMENT, "handle is NULL");
    if (!x) return fail_with(h, QPS_ERR_BAD_ARGUMENT, "qps_polish_shared: x_inout is NULL");
    if (!p) return fail_with(h, QPS_ERR_BAD_ARGUMENT, "qps_polish_shared: params is NULL");
    if (!std::isfinite(p->delta) || std::isnan(p->epsMinres)) return fail_with(h, QPS_ERR_BAD_ARGUMENT, "qps_polish_shared: delta must be finite and epsMinres must not be NaN");
    int rc; SharedFamilyOps* fam = shared_gate(h, "qps_polish_shared", "polish all columns at once (qps_polish serves a stand-alone handle, qps_params.polish a qps_create_dense_batch handle)", &rc);
    if (!fam) return rc;
    const int64_t c = h->fused_batch->count;
    if (!all_finite(x, c * h->n, false)) return fail_with(h, QPS_ERR_BAD_ARGUMENT, "qps_polish_shared: x contains NaN/Inf (the handle is unchanged)");
    if (y && !all_finite(y, c * h->m, false)) return fail_with(h, QPS_ERR_BAD_ARGUMENT, "qps_polish_shared: y contains NaN/Inf (the handle is unchanged)");
    return guarded(h, [&] { fam->polish(x, y, *p, reports); });
}

QPS_API int32_t qps_adjoint_shared(qps_handle hh, const double* x, const double* y, const double* gx, const qps_params* p, double* dq, double* dl, double* du,
                                   double* dP, double* dA, qps_polish_report* reports) {
    Handle* h = reinterpret_cast<Handle*>(hh);
    if (!h) return fail_with(nullptr, QPS_ERR_BAD_ARGUMENT, "handle is NULL");
    if (!x) return fail_with(h, QPS_ERR_BAD_ARGUMENT, "qps_adjoint_shared: x is NULL");
    if (!gx) return fail_with(h, QPS_ERR_BAD_ARGUMENT, "qps_adjoint_shared: gx is NULL");
    if (!p) return fail_with(h, QPS_ERR_BAD_ARGUMENT, "qps_adjoint_shared: params is NULL");
    if (!std::isfinite(p->delta) || std::isnan(p->epsMinres)) return fail_with(h, QPS_ERR_BAD_ARGUMENT, "qps_adjoint_shared: delta must be finite and epsMinres must not be NaN");
    int rc; SharedFamilyOps* fam = shared_gate(h, "qps_adjoint_shared", "differentiate all columns at once", &rc);
    if (!fam) return rc;
    const int64_t c = h->fused_batch->count;
    if (!all_finite(x, c * h->n, false)) return fail_with(h, QPS_ERR_BAD_ARGUMENT, "qps_adjoint_shared: x contains NaN/Inf (the handle is unchanged)");
    if (y && !all_finite(y, c * h->m, false)) return fail_with(h, QPS_ERR_BAD_ARGUMENT, "qps_adjoint_shared: y contains NaN/Inf (the handle is unchanged)");
    if (!all_finite(gx, c * h->n, false)) return fail_with(h, QPS_ERR_BAD_ARGUMENT, "qps_adjoint_shared: gx contains NaN/Inf (the handle is unchanged)");
    return guarded(h, [&] { fam->adjoint(x, y, gx, *p, dq, dl, du, dP, dA, reports); });
}

QPS_API int32_t qps_set_shared_polish(qps_handle hh, int32_t on) {
    Handle* h = reinterpret_cast<Handle*>(hh);
    if (!h) return fail_with(nullptr, QPS_ERR_BAD_ARGUMENT, "handle is NULL");
    if (on != 0 && on != 1) return fail_with(h, QPS_ERR_BAD_ARGUMENT, "qps_set_shared_polish: on must be 0 (qps_solve_batch ends at the loop) or 1 (it ends with the polishing step)");
    int rc; SharedFamilyOps* fam = shared_gate(h, "qps_set_shared_polish", "take this switch (other handles: qps_params.polish)", &rc);
    if (!fam) return rc;
    fam->polish_on = on;
    return QPS_OK;
}

QPS_API int32_t qps_set_shared_equilibration(qps_handle hh, int32_t passes) {
    Handle* h = reinterpret_cast<Handle*>(hh);
    if (!h) return fail_with(nullptr, QPS_ERR_BAD_ARGUMENT, "handle is NULL");
    if (passes < 0 || passes > 50) return fail_with(h, QPS_ERR_BAD_ARGUMENT, "qps_set_shared_equilibration: passes must be in 0..50 (0 switches the scaling off)");
    int rc; SharedFamilyOps* fam = shared_gate(h, "qps_set_shared_equilibration", "are equilibrated", &rc);
    if (!fam) return rc;
    return guarded(h, [&] { fam->set_equilibration(passes); });
}

QPS_API int32_t qps_get_shared_equilibration(qps_handle hh, double* d_out, double* e_out) {
    Handle* h = reinterpret_cast<Handle*>(hh);
    if (!h) return fail_with(nullptr, QPS_ERR_BAD_ARGUMENT, "handle is NULL");
    int rc; SharedFamilyOps* fam = shared_gate(h, "qps_get_shared_equilibration", "are equilibrated", &rc);
    if (!fam) return rc;
    for (int64_t j = 0; d_out && j < h->n; ++j) d_out[j] = fam->eq_kd.empty() ? 1.0 : std::ldexp(1.0, fam->eq_kd[j]);
    for (int64_t i = 0; e_out && i < h->m; ++i) e_out[i] = fam->eq_ke.empty() ? 1.0 : std::ldexp(1.0, fam->eq_ke[i]);
    return QPS_OK;
}

QPS_API int32_t qps_solve_batch_multi(int64_t count, int64_t n, int64_t m, const double* P, const double* A, const double* q, const double* l, const double* u,
                                      int32_t dtype, const int32_t* devices, int32_t num_workers, int32_t chunk, double* x, const qps_params* p, qps_info* infos,
                                      int32_t* worker_of, double* worker_seconds) {
    if (count <= 0 || n <= 0 || m < 0) return fail_with(nullptr, QPS_ERR_BAD_DIMENSION, "need count >= 1, n >= 1 and m >= 0");
    if (!P || !q || !x || (m > 0 && (!A || !l || !u))) return fail_with(nullptr, QPS_ERR_BAD_ARGUMENT, "NULL problem array");
    if (!devices || num_workers <= 0 || num_workers > 256) return fail_with(nullptr, QPS_ERR_BAD_ARGUMENT, "need 1..256 workers and their device list");
    if (chunk > 65535) return fail_with(nullptr, QPS_ERR_BAD_ARGUMENT, "chunk must be at most 65535 (the batch handle's limit)");
    {
        const int rc = validate_params(nullptr, p);
        if (rc != QPS_OK) return rc;
    }
    for (int w = 0; w < num_workers; ++w)
        if (const int dc = require_device(devices[w], "device index out of range in the worker list")) return dc;
    std::mutex err_mu; std::string err_msg; int err_code = QPS_OK;
    auto solve_range = [&](int w, int64_t b0, int64_t cnt) -> int {
        qps_handle h = nullptr;
        int rc = qps_create_dense_batch(cnt, n, m, P + b0 * n * n, A ? A + b0 * m * n : nullptr, q + b0 * n, l ? l + b0 * m : nullptr, u ? u + b0 * m : nullptr, dtype,
                                        devices[w], &h);
        if (rc == QPS_OK) rc = qps_solve_batch(h, x + b0 * n, p, infos ? infos + b0 : nullptr);
        if (rc != QPS_OK) {
            std::lock_guard<std::mutex> lk(err_mu);
            if (err_code == QPS_OK) { err_code = rc; const char* msg = qps_last_error(h); err_msg = msg ? msg : ""; }   // (the message lives on this worker's thread)
        } else if (worker_of) {
            for (int64_t b = b0; b < b0 + cnt; ++b) worker_of[b] = w;
        }
        if (h) (void)qps_destroy(h);
        return rc;
    };
    // one host thread per worker, ranges dealt as batch_schedule.h describes (65535: the batch handle's limit)
    (void)run_batch_workers(count, num_workers, chunk, 65535, solve_range, worker_seconds);
    if (err_code != QPS_OK) return fail_with(nullptr, err_code, err_msg);
    return QPS_OK;
}

QPS_API int32_t qps_set_profiling(qps_handle hh, int32_t on) {
    Handle* h = reinterpret_cast<Handle*>(hh);
    if (!h) return QPS_ERR_BAD_ARGUMENT;
    if (h->impl) { h->impl->prof.level = on; h->impl->prof.reset(); }
    if (h->fused_batch) { h->fused_batch->prof.level = on; h->fused_batch->prof.reset(); }
    for (auto* s : h->batch) { s->prof.level = on; s->prof.reset(); }
    return QPS_OK;
}

QPS_API int32_t qps_kernel_times(qps_handle hh, qps_kernel_time* out, int32_t cap, int32_t* count) {
    Handle* h = reinterpret_cast<Handle*>(hh);
    if (!h || !count) return QPS_ERR_BAD_ARGUMENT;
    SolverBase* s = h->impl ? h->impl : (h->batch.empty() ? nullptr : h->batch[0]);
    Profiler* pf = s ? &s->prof : (h->fused_batch ? &h->fused_batch->prof : nullptr);
    if (!pf) return QPS_ERR_BAD_ARGUMENT;
    int k = 0;
    for (size_t i = 0; i < pf->names.size() && k < cap; ++i) {
        if (pf->stats[i].launches == 0) continue;
        if (out) {
            memset(&out[k], 0, sizeof(out[k]));
            strncpy(out[k].name, pf->names[i].c_str(), sizeof(out[k].name) - 1);
            out[k].seconds = pf->stats[i].seconds; out[k].launches = pf->stats[i].launches; out[k].algo_bytes = pf->stats[i].algo_bytes;
        }
        ++k;
    }
    *count = k;
    return QPS_OK;
}

QPS_API int32_t qps_proxqp_default_params(qps_proxqp_params* p) {
    if (!p) return QPS_ERR_BAD_ARGUMENT;
    memset(p, 0, sizeof(*p));
    p->numIterations = 2000; p->epsAbs = 1e-7; p->epsRel = 1e-6; p->numItrConv = 50; p->rho = 1e2; p->sigma = 1e-2; p->adptRho = 1; p->tau = 10.0;   // ProxQP.jl:118
    return QPS_OK;
}

QPS_API int32_t qps_proxqp_create_dense(int64_t n, int64_t me, int64_t mi, const double* P, int64_t ldp, const double* q, const double* A,
                                        int64_t lda, const double* b, const double* C, int64_t ldc, const double* d, int32_t dtype,
                                        int32_t device, qps_handle* out) {
    if (const int rc = check_out(out)) return rc;
    if (n <= 0 || me < 0 || mi < 0) return fail_with(nullptr, QPS_ERR_BAD_DIMENSION, "need n >= 1, numEq >= 0, numInEq >= 0");
    if (n > (1 << 16) || me + mi > (1 << 20)) return fail_with(nullptr, QPS_ERR_BAD_DIMENSION, "problem too large");
    if (!P || !q || (me > 0 && (!A || !b)) || (mi > 0 && (!C || !d))) return fail_with(nullptr, QPS_ERR_BAD_ARGUMENT, "NULL problem array");
    if (ldp < n || (me > 0 && lda < me) || (mi > 0 && ldc < mi)) return fail_with(nullptr, QPS_ERR_BAD_DIMENSION, "leading dimension smaller than the row count");
    if (const int rc = check_dtype(dtype)) return rc;
    if (const int dc = require_device(device)) return dc;   // this creator alone asks for the device BEFORE finiteness: a NaN without a GPU is NO_DEVICE here
    for (int64_t j = 0; j < n; ++j) {
        if (!all_finite(P + j * ldp, n, false)) return fail_with(nullptr, QPS_ERR_NOT_FINITE, "P contains NaN/Inf");
        if (me > 0 && !all_finite(A + j * lda, me, false)) return fail_with(nullptr, QPS_ERR_NOT_FINITE, "A contains NaN/Inf");
        if (mi > 0 && !all_finite(C + j * ldc, mi, false)) return fail_with(nullptr, QPS_ERR_NOT_FINITE, "C contains NaN/Inf");
    }
    if (!all_finite(q, n, false) || (me > 0 && !all_finite(b, me, false)) || (mi > 0 && !all_finite(d, mi, false)))
        return fail_with(nullptr, QPS_ERR_NOT_FINITE, "q/b/d contain NaN/Inf");
    return create_handle(device, n, me + mi, out, [&](Handle& h) { h.proxqp = make_proxqp(device, n, me, mi, dtype, P, ldp, A, lda, b, C, ldc, d, q); });
}
// SparseProxQP (ProxQP.jl:71, :95-115): the CSC fields of the three SparseMatrixCSC inputs, kept sparse.  The linear system of UpdateX! is solved
// in its KKT form by the sparse L D L' plugin (qps_proxqp.hip: SparseProxQpSolver): symbolic analysis once, a rho update re-factorises numerically
// on the frozen pattern -- the role of AlignSparsePattern / GetNzvalDiagIdxs / UpdateM! / the pattern-reusing cholesky! (:184-190, :201-206, :335-372).
// QPS_PROXQP_SPARSE=0 densifies the inputs onto the dense solver instead (in-place dense re-factorisation, :193-199).
QPS_API int32_t qps_proxqp_create_csc(int64_t n, int64_t me, int64_t mi, const int64_t* Pcp, const int64_t* Pri, const double* Pnz, const double* q,
                                      const int64_t* Acp, const int64_t* Ari, const double* Anz, const double* b, const int64_t* Ccp, const int64_t* Cri,
                                      const double* Cnz, const double* d, int32_t index_base, int32_t dtype, int32_t device, qps_handle* out) {
    if (const int rc = check_out(out)) return rc;
    if (n <= 0 || me < 0 || mi < 0) return fail_with(nullptr, QPS_ERR_BAD_DIMENSION, "need n >= 1, numEq >= 0, numInEq >= 0");
    if (!Pcp || !q || (me > 0 && (!Acp || !b)) || (mi > 0 && (!Ccp || !d))) return fail_with(nullptr, QPS_ERR_BAD_ARGUMENT, "NULL problem array");
    if (index_base != 0 && index_base != 1) return fail_with(nullptr, QPS_ERR_BAD_ARGUMENT, "index_base must be 0 or 1");
    if (const int rc = check_dtype(dtype)) return rc;
    auto validate = [&](const int64_t* cp, const int64_t* ri, const double* nz, int64_t rows, const char* name) -> int {
        if (rows == 0) return QPS_OK;
        if (cp[0] != index_base) return fail_with(nullptr, QPS_ERR_BAD_ARGUMENT, std::string(name) + ": colptr does not start at index_base");
        for (int64_t j = 0; j < n; ++j) if (cp[j + 1] < cp[j]) return fail_with(nullptr, QPS_ERR_BAD_ARGUMENT, std::string(name) + ": colptr not monotone");
        const int64_t nnz = cp[n] - index_base;
        if (nnz > 0 && (!ri || !nz)) return fail_with(nullptr, QPS_ERR_BAD_ARGUMENT, std::string(name) + ": NULL index / value array");
        for (int64_t k = 0; k < nnz; ++k) {
            const int64_t i = ri[k] - index_base;
            if (i < 0 || i >= rows) return fail_with(nullptr, QPS_ERR_BAD_DIMENSION, std::string(name) + ": row index out of range");
        }
        if (!all_finite(nz, nnz, false)) return fail_with(nullptr, QPS_ERR_NOT_FINITE, std::string(name) + " contains NaN/Inf");
        return QPS_OK;
    };
    int rv = validate(Pcp, Pri, Pnz, n, "mP"); if (rv == QPS_OK) rv = validate(Acp, Ari, Anz, me, "mA"); if (rv == QPS_OK) rv = validate(Ccp, Cri, Cnz, mi, "mC");
    if (rv != QPS_OK) return rv;
    static const bool keep_sparse = [] { const char* e = getenv("QPS_PROXQP_SPARSE"); return !(e && atoi(e) == 0); }();
    if (keep_sparse && me + mi > 0) {
        if (n > 2000000000LL || me + mi > 2000000000LL) return fail_with(nullptr, QPS_ERR_BAD_DIMENSION, "problem too large");
        if (!all_finite(q, n, false) || (me > 0 && !all_finite(b, me, false)) || (mi > 0 && !all_finite(d, mi, false)))
            return fail_with(nullptr, QPS_ERR_NOT_FINITE, "q/b/d contain NaN/Inf");
        return create_handle(device, n, me + mi, out, [&](Handle& h) {
            h.proxqp = make_proxqp_sparse(device, n, me, mi, dtype, Pcp, Pri, Pnz, q, Acp, Ari, Anz, b, Ccp, Cri, Cnz, d, index_base);
        });
    }
    if (n > (1 << 16) || me + mi > (1 << 20)) return fail_with(nullptr, QPS_ERR_BAD_DIMENSION, "problem too large to densify");
    const std::vector<double> Pd = densify_csc(Pcp, Pri, Pnz, n, n, index_base), Ad = densify_csc(Acp, Ari, Anz, me, n, index_base),
                              Cd = densify_csc(Ccp, Cri, Cnz, mi, n, index_base);
    return qps_proxqp_create_dense(n, me, mi, Pd.data(), n, q, me > 0 ? Ad.data() : nullptr, std::max<int64_t>(me, 1), b, mi > 0 ? Cd.data() : nullptr,
                                   std::max<int64_t>(mi, 1), d, dtype, device, out);
}
QPS_API int32_t qps_proxqp_init_kkt(qps_handle hh) {
    Handle* h = reinterpret_cast<Handle*>(hh);
    if (!h || !h->proxqp) return fail_with(h, QPS_ERR_BAD_ARGUMENT, "not a ProxQP handle");
    return guarded(h, [&] { h->proxqp->init_kkt(); });
}
QPS_API int32_t qps_proxqp_set_state(qps_handle hh, const double* x, const double* y, const double* z, const double* s) {
    Handle* h = reinterpret_cast<Handle*>(hh);
    if (!h || !h->proxqp) return fail_with(h, QPS_ERR_BAD_ARGUMENT, "not a ProxQP handle");
    if (!x || (h->proxqp->me > 0 && !y) || (h->proxqp->mi > 0 && (!z || !s))) return fail_with(h, QPS_ERR_BAD_ARGUMENT, "NULL state vector");
    return guarded(h, [&] { h->proxqp->set_state(x, y, z, s); });
}
QPS_API int32_t qps_proxqp_get_state(qps_handle hh, double* x, double* y, double* z, double* s) {
    Handle* h = reinterpret_cast<Handle*>(hh);
    if (!h || !h->proxqp) return fail_with(h, QPS_ERR_BAD_ARGUMENT, "not a ProxQP handle");
    return guarded(h, [&] { h->proxqp->get_state(x, y, z, s); });
}
QPS_API int32_t qps_proxqp_solve(qps_handle hh, const qps_proxqp_params* p, qps_proxqp_report* rep) {
    Handle* h = reinterpret_cast<Handle*>(hh);
    if (!h || !h->proxqp) return fail_with(h, QPS_ERR_BAD_ARGUMENT, "not a ProxQP handle");
    if (!p) return fail_with(h, QPS_ERR_BAD_ARGUMENT, "params is NULL");
    if (p->numIterations < 0 || p->numItrConv <= 0 || !(p->rho > 0) || !(p->sigma >= 0) || !(p->tau > 0))
        return fail_with(h, QPS_ERR_BAD_ARGUMENT, "need numIterations >= 0, numItrConv > 0, rho > 0, sigma >= 0, tau > 0");
    return guarded(h, [&] { h->proxqp->solve(*p, rep); });
}

QPS_API int32_t qps_linsys_auto(int64_t n, int64_t m, int64_t nnzP, int64_t nnzA, int32_t sparse_input) {
    // SolveQuadraticProgram.jl:129-130 MAX_NUM_ROWS_L = 5000, MAX_DENSITY = 0.4; :143-151 (SolveQuadraticProgram.m:190-199)
    const double numRowsL = (double)n + (double)m;
    const double nnzDensity = ((double)nnzP + (double)nnzA) / (numRowsL * numRowsL);
    const bool directSol = (numRowsL <= 5000.0) && (nnzDensity <= 0.4);
    if (!directSol) return QPS_LINSYS_CG;
    return sparse_input ? QPS_LINSYS_KKT_LDL : QPS_LINSYS_CHOLESKY;
}

QPS_API int32_t qps_ldl_analyze(int64_t n, int64_t m, const int64_t* Pcp, const int64_t* Pri, const int64_t* Acp, const int64_t* Ari,
                                int32_t index_base, int64_t* perm_out, qps_ldl_report* rep) {
    if (n <= 0 || m < 0 || n + m > 2000000000LL) return fail_with(nullptr, QPS_ERR_BAD_DIMENSION, "need n >= 1, m >= 0, n + m < 2^31");
    if (!Pcp || !Acp || (!Pri && Pcp[n] > index_base) || (!Ari && Acp[n] > index_base)) return fail_with(nullptr, QPS_ERR_BAD_ARGUMENT, "NULL index array");
    if (index_base != 0 && index_base != 1) return fail_with(nullptr, QPS_ERR_BAD_ARGUMENT, "index_base must be 0 or 1");
    for (int64_t j = 0; j < n; ++j) if (Pcp[j + 1] < Pcp[j] || Acp[j + 1] < Acp[j]) return fail_with(nullptr, QPS_ERR_BAD_ARGUMENT, "colptr not monotone");
    for (int64_t k = 0; k < Pcp[n] - index_base; ++k) if (Pri[k] - index_base < 0 || Pri[k] - index_base >= n) return fail_with(nullptr, QPS_ERR_BAD_DIMENSION, "P row index out of range");
    for (int64_t k = 0; k < Acp[n] - index_base; ++k) if (Ari[k] - index_base < 0 || Ari[k] - index_base >= m) return fail_with(nullptr, QPS_ERR_BAD_DIMENSION, "A row index out of range");
    return guarded(nullptr, [&] {
        const LdlLimits lim = ldl_limits_from_env();
        LdlSymbolic s;
        try { s = ldl_analyze((int)n, (int)m, Pcp, Pri, Acp, Ari, index_base, lim.max_tail, lim.min_level_width, lim.max_levels); }
        catch (const std::runtime_error& e) { throw QpsError(QPS_ERR_UNSUPPORTED, e.what()); }
        if (perm_out) for (int64_t k = 0; k < n + m; ++k) perm_out[k] = (int64_t)s.perm[k] + index_base;
        if (rep) {
            rep->numRows = s.N; rep->numSparseColumns = s.Ns; rep->tailSize = s.Nt; rep->numSparseLevels = (int64_t)s.level_ptr.size() - 1;
            rep->treeHeight = s.levels_total; rep->nnzK = s.nnzK; rep->nnzL = s.nnzL_exact; rep->nnzStored = s.nnzL;
        }
    });
}

QPS_API int32_t qps_destroy(qps_handle hh) {
    Handle* h = reinterpret_cast<Handle*>(hh);
    delete h;   // (NULL: nothing to do)
    return QPS_OK;
}

QPS_API const char* qps_last_error(qps_handle hh) {
    Handle* h = reinterpret_cast<Handle*>(hh);
    if (h) return h->err.c_str();
    return g_last_error.c_str();
}

QPS_API const char* qps_version(void) { return "qps-hip 0.1 (gfx950)"; }

}  // extern "C"
