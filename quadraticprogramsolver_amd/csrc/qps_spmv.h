// qps_spmv.h -- the CSR products and the CG plugin built on them (internal).  The kernels and the objects that launch them are in k_sparse.hip;
// the drivers composed from them are SparseSolver (qps_sparse.hip) and SparseProxQpSolver (qps_proxqp.hip).
#pragma once
#include <cstdint>
#include <memory>

#include "qps_internal.h"
#include "qps_kernels.h"
#include "qps_ldl.h"
#include "spmv_layout.h"

namespace qps {

struct CgState { double res2, prev2, tol, uc; int iters, done, maxiter, pad; };   // two copies, ping-ponged per CG iteration

struct Csr {
    int nrows = 0; int64_t nnz = 0; int* rp = nullptr; int* ci = nullptr; void* va = nullptr; int* rb = nullptr; int nblocks = 0;
    // column-blocked copy (k_spmv_blk): nblk CSR blocks back to back; used when `blocked`
    bool blocked = false; int ncols = 0, nblk = 0, wpb = 0; int* brp = nullptr; unsigned short* bci = nullptr; void* bva = nullptr;
    int* task_ptr = nullptr; int4* tasks = nullptr; int per = 1, lpr4 = 0; void* partial = nullptr;
    int* lr_ptr = nullptr; int4* lr_desc = nullptr;   // rows with more than BCHUNK entries in one block: (row, first entry, end entry, 0), [nblk + 1] ranges
    // sliced form (k_spmv_sell): units of 64 lanes x E entries; bci / bva then hold only the long rows' entries
    bool sell = false; int nsl = 0, win = layout::SIGMA, nwin = 0, staged = 0; int* wg_ptr = nullptr; int* sl_off = nullptr; unsigned short* sl_perm = nullptr; void* s_cols = nullptr; void* s_vals = nullptr;
    // value refresh of a matrix with a frozen pattern (the explicit reduced matrix): where every slot of s_vals / bva came from in `va`
    int* src = nullptr; int64_t src_n = 0; int* lsrc = nullptr; int64_t lsrc_n = 0;
};

// out = a * (M in) + b0 add0 + b1 add1; optional partial[workgroup of the last launch] = sum_rows dotv[row] * out[row].  stt: a CG iteration enqueued past
// convergence returns at its first instruction.
template <typename T> struct SpmvEpilogue {
    T a = T(1); const T* add0 = nullptr; T b0 = T(0); const T* add1 = nullptr; T b1 = T(0);
    const T* dotv = nullptr; double* partial = nullptr; const CgState* stt = nullptr;
};

// The pinned read-back block of a CSC handle (kPinnedBytes, qps_internal.h): who reads what where
constexpr size_t kPinCgState = 0;          // CgState[2]: the state after a batch of CG iterations | the initial residual
constexpr size_t kPinCheck = 128;          // 8 doubles of check_convergence
constexpr size_t kPinProxQpSlots = 256;    // 12 words of k_pq_norms
static_assert(kPinCgState + 2 * sizeof(CgState) <= kPinCheck && kPinCheck + 8 * sizeof(double) <= kPinProxQpSlots && kPinProxQpSlots + 12 * sizeof(unsigned long long) <= kPinnedBytes,
              "regions of the pinned block overlap");

// The matrices of a CSC handle on the device -- P, A and A' as CSR, each with its column-blocked copy when that pays -- with the stream they are multiplied on,
// the owner of every device buffer of the handle and the staging buffer of its vector transfers.
template <typename T> struct SparseMatrices {
    // destroyed in reverse: the buffers, then the stream lease (what works on the stream is declared after this object by its owner, and goes first)
    StreamLease lease; DeviceOwner mem; std::unique_ptr<StagedUploader> up;   // `up` lives for the duration of the owner's constructor (and of explicit_prepare) only
    int device = 0; hipStream_t st = nullptr; int64_t n = 0, m = 0;
    Csr A, At, P;
    double* stage = nullptr;

    SparseMatrices(int device, int64_t n, int64_t m);                          // stream + pinned block, the uploader opened, the staging buffer
    void load(const layout::CsrHost& Ph, const layout::CsrHost& Ah, const layout::CsrHost& Ath);
    template <typename V> V* upload_array(const std::vector<V>& v, int64_t min_count = 1) {
        V* d = mem.dalloc<V>(std::max<int64_t>((int64_t)v.size(), min_count), st);
        if (!v.empty()) up->copy(d, v.data(), sizeof(V) * v.size());
        return d;
    }
    void build_blocked(Csr& M, const layout::CsrHost& H, bool with_src = false);
    void upload_csr(Csr& M, const layout::CsrHost& H, bool with_src = false);
    void upload_vec(const double* h, T* d, int64_t count) { HIPC(upload_staged<T>(st, stage, h, d, count)); }
    void download_vec(const T* d, double* h, int64_t count) { HIPC(download_staged<T>(st, stage, d, h, count)); }
    CgState* cg_state_host() const { return reinterpret_cast<CgState*>(static_cast<char*>(lease.res.pinned) + kPinCgState); }
    double* check_host() const { return reinterpret_cast<double*>(static_cast<char*>(lease.res.pinned) + kPinCheck); }
    unsigned long long* proxqp_slots_host() const { return reinterpret_cast<unsigned long long*>(static_cast<char*>(lease.res.pinned) + kPinProxQpSlots); }

    void mul(const Csr& M, const T* in, T* out) { mul(M, in, out, SpmvEpilogue<T>()); }         // out = M in
    void mul(const Csr& M, const T* in, T* out, const SpmvEpilogue<T>& e);
    void axpby(int64_t count, T a, const T* x, T b, const T* y, T* out);                        // out = a x + b y; count <= 0 does nothing
};

// ItrSolCgInit / ItrSolCg! (LinearSystemSolvers.jl:110-142): the explicit reduced matrix mL = mPI + rho mAA on a frozen pattern; ONE product per CG iteration
template <typename T> struct ReducedMatrix {
    Csr mat; T *vP = nullptr, *vAA = nullptr, *dg = nullptr;   // mP, mAA and the identity as value arrays on mat's pattern (k_build_reduced combines them)
    int state = 0;                   // 0 undecided, 1 built, -1 declined (too dense to pay, or its inputs were released)
    bool valid = false; double rho = 0, sigma = 0;             // what mat's values were last built for
};

// The CG plugin: LinOpCg (LinearSystemSolvers.jl:145-186, the matrix-free reduced operator) and ItrSolCg (:110-142, the explicit reduced matrix).
template <typename T> struct CgPlugin {
    SparseMatrices<T>& M; Profiler& prof;
    Csr PA;   // PA = [P; A] stacked, column-blocked only: P u and A u of the CG operator from ONE pass over u
    ReducedMatrix<T> L; bool cg_explicit = false;   // cg_explicit: the current request is served by L
    T *cu = nullptr, *cu2 = nullptr, *cr = nullptr, *cc = nullptr, *tm = nullptr;                // n, n, n, n, m
    double *part_uc = nullptr, *part_rr = nullptr; int part_uc_cap = 0; CgState* state = nullptr;
    int nb_n = 0; int64_t cg_total = 0; int last_cg = 4;
    double eps_pcg = 1e-6; int itr_pcg = 1000;
    int cat_op = 0, cat_pa = 0, cat_at = 0; int prof_calls = 0;                                 // profiler categories, registered by the driver

    CgPlugin(SparseMatrices<T>& mats, Profiler& prof_) : M(mats), prof(prof_) {}
    void build(const layout::CsrHost& Ph, const layout::CsrHost& Ah);          // the stacked [P; A] when all three products are blocked; the vectors
    bool explicit_prepare(bool forced, const KktPlugin<T>& kkt);
    void reduced_values(double rho, double sigma);
    int resolve_cg(int linsys, double rho, double sigma, const KktPlugin<T>& kkt);
    void op_reduced(const T* uin, T* cout, double rho, double sigma, double* partial, const CgState* stt);
    void stacked_product(const T* uin, T* both);                               // both = [P; A] u through the stacked copy (PA.blocked)
    int cg(double rho, double sigma, const T* tt, T* xx);                      // xx warm started; returns the iteration count
};

}  // namespace qps
