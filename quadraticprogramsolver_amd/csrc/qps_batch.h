// qps_batch.h -- what the batch handles share between qps_capi.hip (handle plumbing), qps_dense_batch.hip (BatchedDenseSolver) and the shared-matrix family
// (qps_shared_family.h: the driver; qps_shared_dense.hip, qps_shared_csr.hip: its three paths): the base of every fused batch solver, the one interface the qps_*_shared_* entry points talk to, the factories of all three, and the
// panelled matrix upload.
#pragma once
#include "ldl_symbolic.h"
#include "qps_internal.h"
#include "qps_kernels.h"

namespace qps {

// One matrix of qps_update_shared_matrices_csc after layout::canonical_csc (0-based, rows sorted, duplicates summed); given == false keeps the handle's matrix
struct CanonicalCsc { bool given = false; std::vector<int64_t> cp, ri; std::vector<double> nz; };

// What the device found in the staged values of qps_update_shared_values, in the order the host tests of qps_update_shared_matrices_csc run in
struct ValuesVerdict {
    const char* not_finite = nullptr;    // "P" / "A": the first matrix that holds a NaN or an Inf
    int64_t asymmetric_column = -1;      // the column layout::csc_asymmetry names for these values of P
    bool refused() const { return not_finite || asymmetric_column >= 0; }
};

// What only the shared-matrix batches take (qps_update_shared_vectors, qps_set_shared_*, qps_get_shared_equilibration); arrays validated by the caller.
struct SharedFamilyOps {
    int family_rho = 0;               // qps_set_shared_adaptive_rho: 0 fixed rho, 1 the family rule (one factor, hence one rho to move)
    int column_rho = 0;               // qps_set_shared_column_rho: 1 every column moves its own rho (a path without a factor only: takes_column_rho)
    int warm_start = 0;               // qps_set_shared_warm_start: 0 z = y = 0, 1 the stored (z, y), 2 z = A x and the stored y
    int polish_on = 0;                // qps_set_shared_polish: 1 = every solve_batch ends with the polishing step on its own x and y
    std::vector<int> eq_kd, eq_ke;    // qps_set_shared_equilibration: D_j = 2^eq_kd[j], E_i = 2^eq_ke[i]; empty while off
    virtual ~SharedFamilyOps() {}
    virtual void update_vectors(const double* q, const double* l, const double* u) = 0;   // [count][n], [count][m], [count][m]; NULL keeps that array
    virtual bool takes_column_rho() const { return false; }                               // rho is a multiplier of the path, not part of a factor
    virtual void set_rho_scale(const double* scale) = 0;                                  // [m], or NULL
    virtual void set_equilibration(int passes) = 0;                                       // 0..50
    virtual void set_dual(const double* z, const double* y) = 0;                          // [count][m] each, finite; NULL keeps that array
    virtual void set_infeasibility(double epsPrimInf, double epsDualInf) = 0;             // qps_set_shared_infeasibility: finite, >= 0; both 0 = off
    virtual void get_certificate(double* dy, double* dx) = 0;                             // [count][m], [count][n]; either may be NULL
    // qps_polish_shared: x [count][n] (replaced where reports[b].flag == 0), y [count][m] or NULL = the stored y, reports [count] or NULL; finite arrays
    virtual void polish(double* x, const double* y, const qps_params& p, qps_polish_report* reports) = 0;
    // qps_adjoint_shared: x, gx [count][n], y [count][m] or NULL = the stored y, finite arrays; dq [count][n], dl, du [count][m], dP [nnz(P)], dA [nnz(A)] and
    // reports [count] may each be NULL.  Nothing the handle keeps is written.
    virtual void adjoint(const double* x, const double* y, const double* gx, const qps_params& p, double* dq, double* dl, double* du, double* dP, double* dA,
                         qps_polish_report* reports) = 0;
    // qps_update_shared_matrices / qps_update_shared_matrices_csc: new values on the handle's pattern, everything else kept (options, q, l, u, z, y, analysis,
    // allocations); the numeric factor goes stale.  A path implements the form it was created from; the other form is refused with QPS_ERR_UNSUPPORTED before the
    // arrays are looked at (takes_csc() tells qps_capi.hip which).  A refused call leaves the handle bit for bit what it was; a returning call leaves the stream idle.
    virtual bool takes_csc() const = 0;
    virtual void update_matrices(const double* P, int64_t ldp, const double* A, int64_t lda) = 0;   // column-major, NULL keeps that matrix
    virtual void update_matrices_csc(const CanonicalCsc& P, const CanonicalCsc& A) = 0;             // pattern compared with the handle's, entry for entry
    // qps_get_shared_pattern: the canonical pattern of a path that takes CSC (the dense path refuses); any output may be NULL
    virtual void get_pattern(int64_t* nnzP, int64_t* nnzA, int64_t* Pcp, int64_t* Pri, int64_t* Acp, int64_t* Ari) = 0;
    // qps_update_shared_values: new values in the order of that pattern, from host (location 0) or device memory (1); NULL keeps that matrix.  The values are
    // staged and tested on the device before anything of the handle is touched.  A verdict other than the default one is a refusal that qps_capi.hip words with
    // the texts of the creators (nothing was modified); every other refusal is thrown.
    virtual ValuesVerdict update_values(const double* P, int64_t nnzP, const double* A, int64_t nnzA, int location) = 0;
};

struct BatchSolverBase {
    int device = 0; int64_t n = 0, m = 0; int count = 0; std::string err; Profiler prof;
    virtual ~BatchSolverBase() {}
    virtual void solve_batch(double* x, const qps_params& p, qps_info* infos) = 0;
    virtual void get_dual(double* z, double* y) = 0;   // [count][m] each
    virtual SharedFamilyOps* shared_family() { return nullptr; }   // the shared-matrix batches only
};

// `count` independent dense QPs of one shape in lock step (qps_dense_batch.hip): P [count][n * n], A [count][m * n] column-major, q [count][n], l / u [count][m],
// validated by the caller.  The loaded solver, or nullptr when the fused pass does not cover the shape (count = 1, m = 0, n beyond its limit).
BatchSolverBase* make_dense_batch(int device, int dtype, int count, int64_t n, int64_t m, const double* P, const double* A, const double* q, const double* l,
                                  const double* u);

struct SparseSharedInput {   // what qps_create_csc_shared_batch prepares on the host before a device is needed
    LdlSymbolic sym; std::vector<int64_t> Pcp, Pri, Acp, Ari; std::vector<double> Pnz, Anz; int spr = 0;
};
struct CgSharedInput {       // what qps_create_csc_shared_batch_cg prepares on the host: the canonical CSC arrays (0-based, rows sorted, duplicates summed)
    std::vector<int64_t> Pcp, Pri, Acp, Ari; std::vector<double> Pnz, Anz;
};
int shared_batch_max_np(int dtype);   // the largest padded n of a dense shared-matrix batch
BatchSolverBase* make_dense_shared_batch(int device, int dtype, int count, int64_t n, int64_t m, const double* P, int64_t ldp, const double* A, int64_t lda,
                                         const double* q, const double* l, const double* u);
BatchSolverBase* make_sparse_shared_batch(int device, int dtype, int count, int64_t n, int64_t m, SparseSharedInput&& in, const double* q, const double* l,
                                          const double* u);
BatchSolverBase* make_cg_shared_batch(int device, int dtype, int count, int64_t n, int64_t m, CgSharedInput&& in, const double* q, const double* l, const double* u);

// column-major host matrix (rows x cols, ld ldh) -> row-major device T (ld ldd), streamed through a bounded device staging buffer in column panels
template <typename T>
inline void upload_matrix_panels(hipStream_t st, int device, const double* h, int64_t ldh, int rows, int cols, T* d, int64_t ldd) {
    if (rows <= 0 || cols <= 0) return;
    const int64_t budget = (int64_t)32 << 20;   // doubles per panel (256 MiB)
    int pc = (int)std::max<int64_t>(64, (budget / std::max(rows, 1)) / 64 * 64);
    DeviceOwner tmp_mem;
    double* buf = tmp_mem.alloc<double>((int64_t)rows * std::min(pc, cols));
    FastUploader fu(st, device);                 // pinned ring filled by several host threads (qps_internal.h)
    for (int c0 = 0; c0 < cols; c0 += pc) {
        const int nc = std::min(pc, cols - c0);
        if (ldh == rows) fu.copy(buf, h + (int64_t)c0 * ldh, sizeof(double) * (size_t)rows * (size_t)nc);
        else for (int c = 0; c < nc; ++c) fu.copy(buf + (int64_t)c * rows, h + (int64_t)(c0 + c) * ldh, sizeof(double) * (size_t)rows);
        import_colmajor<T>(st, buf, rows, rows, nc, d + c0, ldd);
        HIPC(hipStreamSynchronize(st));
    }
}

}  // namespace qps
