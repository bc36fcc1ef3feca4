// qps_proxqp.hip -- the reference's second solver form (ProxQP.jl) on the same device kernels.
//
//     min 1/2 x'Px + q'x   s.t.  A x = b,  C x <= d                               (ProxQP.jl:118-124)
//
// With the stacked constraint matrix G = [A; C] the iteration of ProxQP.jl:135-149 is the ADMM skeleton of the main path:
//     M = P + sigma I + rho G'G  (UpdateM! :175-181)      ->  same assembly + Cholesky + sweep matrix as DenseSolver
//     r = sigma x - q + G'w,  w = [rho b - y ; rho (d - s) - z]   (CalculateRhs! :208-219)
//     x = M^{-1} r                                          (UpdateX! :221-225)   ->  fused sweeps
//     v = G x;  s = max(d - z/rho - v, 0) (:227-233);  y += rho (v - b) (:235-240);  z = max(z + rho (s - d) + rho v, 0) (:242-249)
// CheckConvergence! (:252-298) runs every numItrConv iterations; the loop never breaks on convergence (:156).
// The dense convenience constructor's initialisation (:73-93: x, y from the equality-constrained KKT system) is done on the
// device by the range-space method: x = -P^{-1}(q + A'y), (A P^{-1} A') y = -(b + A P^{-1} q).
// The same form on CSC inputs follows the dense one below: its linear system in KKT form, on the sparse products (qps_spmv.h) and the L D L' plugin (qps_ldl.h).
#include <algorithm>
#include <memory>

#include "dense_chol.h"
#include "qps_internal.h"
#include "qps_kernels.h"
#include "qps_ldl.h"
#include "qps_proxqp.h"
#include "qps_spmv.h"
#include "k_proxqp_rows.h"

namespace qps {

namespace {

using namespace pqrows;

template <typename T> __global__ void k_pq_scale_add(int n, T a, const T* __restrict__ x, T b, const T* __restrict__ y, T* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = a * x[i] + (y ? b * y[i] : T(0));
}
// dst = lower triangle of src (upper zero): the sweep matrix without its mirrored half, usable as a plain GEMM operand
template <typename T> __global__ void k_pq_lower(int NP, const T* __restrict__ src, T* __restrict__ dst) {
    const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
    if (j < NP) dst[(int64_t)i * NP + j] = (j <= i) ? src[(int64_t)i * NP + j] : T(0);
}

inline dim3 g1(int n) { return dim3((unsigned)((std::max(n, 1) + 255) / 256)); }

template <typename T> struct ProxQpSolver : ProxQpBase {
    StreamLease lease; DeviceOwner mem; hipStream_t st = nullptr;   // destroyed in reverse: buffers first, then the stream lease
    int NP = 0, MP = 0, MEP = 0, mtot = 0, nb = 0, part_tiles = 0;
    T *G = nullptr, *Aonly = nullptr, *P = nullptr, *q = nullptr, *g = nullptr, *dual = nullptr, *slack = nullptr, *x = nullptr;
    T *w = nullptr, *v = nullptr, *de = nullptr, *di = nullptr, *tt = nullptr, *yv = nullptr, *xx = nullptr, *part = nullptr, *sw_part = nullptr;
    T *PI = nullptr, *KK = nullptr, *M = nullptr, *S = nullptr, *tmp = nullptr, *dinv = nullptr, *X1 = nullptr, *X2 = nullptr, *X3 = nullptr;
    int* fail = nullptr; unsigned long long* slots = nullptr; unsigned long long* slots_host = nullptr; double* stage = nullptr;
    bool have_K = false;

    ProxQpSolver(int dev, int64_t n_, int64_t me_, int64_t mi_) {
        device = dev; n = n_; me = me_; mi = mi_;
        HIPC(hipSetDevice(device));
        st = lease.acquire(device);   // recycled stream + pinned block (qps_internal.h)
        mtot = (int)(me + mi);
        NP = roundup(n, 64); MP = roundup(mtot, 64); MEP = roundup(std::max<int64_t>(me, 1), 64);
        const int64_t nn = (int64_t)NP * NP;
        G = mem.dalloc<T>((int64_t)MP * NP, st); Aonly = mem.dalloc<T>((int64_t)MEP * NP, st); P = mem.dalloc<T>(nn, st); q = mem.dalloc<T>(NP, st); x = mem.dalloc<T>(NP, st);
        g = mem.dalloc<T>(MP, st); dual = mem.dalloc<T>(MP, st); slack = mem.dalloc<T>(MP, st); w = mem.dalloc<T>(MP, st); v = mem.dalloc<T>(MP, st); de = mem.dalloc<T>(MP, st); di = mem.dalloc<T>(MP, st);
        tt = mem.dalloc<T>(NP, st); yv = mem.dalloc<T>(NP, st); xx = mem.dalloc<T>(NP, st); X1 = mem.dalloc<T>(NP, st); X2 = mem.dalloc<T>(NP, st); X3 = mem.dalloc<T>(NP, st);
        part_tiles = std::max(gemv_cols_tiles(MP), apass_proxqp_slabs<T>(NP, MP));
        part = mem.dalloc<T>((int64_t)std::max(part_tiles, 1) * NP, st);
        sw_part = mem.dalloc<T>((int64_t)std::max(sweep_fused_slabs<T>(NP), 1) * NP, st);
        PI = mem.dalloc<T>(nn, st); KK = mem.dalloc<T>(nn, st); M = mem.dalloc<T>(nn, st); S = mem.dalloc<T>(nn, st); tmp = mem.dalloc<T>(nn, st); dinv = mem.dalloc<T>((int64_t)(NP / 64) * 4096, st);
        fail = mem.dalloc<int>(4, st); slots = mem.dalloc<unsigned long long>(16, st);
        slots_host = reinterpret_cast<unsigned long long*>(lease.res.pinned);
        stage = mem.dalloc<double>(std::max<int64_t>((int64_t)MP * NP, nn) + 64, st);
    }
    ~ProxQpSolver() override {
        (void)hipSetDevice(device);
        (void)hipStreamSynchronize(st);
    }
    void put_vec(const double* h, T* d, int64_t c) { HIPC(upload_staged<T>(st, stage, h, d, c)); }
    void get_vec(const T* d, double* h, int64_t c) { HIPC(download_staged<T>(st, stage, d, h, c)); }
    void put_matrix(const double* h, int64_t ldh, int rows, int cols, T* d) {   // column-major host -> row-major device rows (ld NP)
        if (rows <= 0 || cols <= 0) return;
        HIPC(hipMemcpy2DAsync(stage, sizeof(double) * (size_t)rows, h, sizeof(double) * (size_t)ldh, sizeof(double) * (size_t)rows, (size_t)cols, hipMemcpyHostToDevice, st));
        import_colmajor<T>(st, stage, rows, rows, cols, d, NP);
        HIPC(hipStreamSynchronize(st));
    }
    void load(const double* Ph, int64_t ldp, const double* Ah, int64_t lda, const double* bh, const double* Ch, int64_t ldc, const double* dh, const double* qh) {
        put_matrix(Ph, ldp, (int)n, (int)n, P);
        put_matrix(Ah, lda, (int)me, (int)n, G);
        put_matrix(Ah, lda, (int)me, (int)n, Aonly);
        put_matrix(Ch, ldc, (int)mi, (int)n, G + (int64_t)me * NP);
        put_vec(qh, q, n); put_vec(bh, g, me); put_vec(dh, g + me, mi);
    }
    DenseChol<T> chol() const { return {st, (int)n, NP, MP, P, G, PI, KK, M, S, tmp, dinv, fail}; }

    // UpdateDecomposition! (ProxQP.jl:193-199): M = P + rho K + sigma I, Cholesky, sweep matrix
    void update_decomposition(double rho, double sigma) {
        const DenseChol<T> c = chol();
        c.form(sigma, rho, true, !have_K);                                                          // mK = A'A + C'C (:42-46) once, :178-180
        have_K = true;
        nb = pick_nb<T>(0, NP);
        c.factor(nb);                                                                               // :196
        int f = 0;
        c.check("P + rho (A'A + C'C) + sigma I", "", &f);
    }

    void set_state(const double* xh, const double* yh, const double* zh, const double* sh) override {
        HIPC(hipSetDevice(device));
        put_vec(xh, x, n); put_vec(yh, dual, me); put_vec(zh, dual + me, mi);
        HIPC(hipMemsetAsync(slack, 0, sizeof(T) * MP, st));
        put_vec(sh, slack + me, mi);
    }
    void get_state(double* xh, double* yh, double* zh, double* sh) override {
        HIPC(hipSetDevice(device));
        if (xh) get_vec(x, xh, n);
        if (yh) get_vec(dual, yh, me);
        if (zh) get_vec(dual + me, zh, mi);
        if (sh) get_vec(slack + me, sh, mi);
    }

    // ProxQP.jl:73-93 on the device (range-space method; P is SPD as the reference requires, A needs full row rank)
    void init_kkt() override {
        HIPC(hipSetDevice(device));
        const DenseChol<T> cP = chol();
        const int nbP = pick_nb<T>(0, NP);
        int f = 0;
        make_PI<T>(st, (int)n, NP, P, T(0), PI);                     // P with identity on the padding
        HIPC(hipMemcpyAsync(M, PI, sizeof(T) * (size_t)NP * NP, hipMemcpyDeviceToDevice, st));
        cP.factor(nbP);                                              // S: sweep matrix of P
        cP.check("P (KKT initialisation)", "", &f);
        HIPC(hipMemsetAsync(dual, 0, sizeof(T) * MP, st));
        if (me > 0) {
            if (nbP < NP) throw QpsError(QPS_ERR_UNSUPPORTED, "KKT initialisation of the dense solver needs n <= 16384 fp64 / 32768 fp32 (pass an explicit state, or CSC inputs for the sparse solver)");
            // B = W_P A'  (NP x MEP), W_P = inv(L_P) = lower triangle of S ; Schur = B'B = A P^{-1} A'
            T* Wl = tmp;                                             // lower-only copy of the sweep matrix
            hipLaunchKernelGGL((k_pq_lower<T>), dim3((NP + 255) / 256, NP), dim3(256), 0, st, NP, S, Wl);
            T* B = PI;                                               // reuse: NP x MEP (<= NP x NP needs MEP <= NP)
            T* Sch = KK; have_K = false;                             // MEP x MEP, ld MEP
            if (MEP > NP) throw QpsError(QPS_ERR_UNSUPPORTED, "KKT initialisation needs numEq <= n");
            gemm<T>(st, NP, MEP, NP, T(1), Wl, NP, true, Aonly, NP, true, T(0), B, MEP, false, 1, 0, 0, 0, 2);
            gemm<T>(st, MEP, MEP, NP, T(1), B, MEP, false, B, MEP, false, T(0), Sch, MEP, false);
            T* SchPI = M;                                            // Schur + identity on its padding
            make_PI<T>(st, (int)me, MEP, Sch, T(0), SchPI);
            DenseChol<T> cS = cP;                                    // the Schur factor: order MEP, its sweep matrix in Wl (no longer needed
            cS.NP = MEP; cS.M = SchPI; cS.S = Wl; cS.tmp = B;         // after the two GEMMs), B as scratch, dinv and fail shared with P's
            const int nb2 = pick_nb<T>(0, MEP);
            cS.factor(nb2);
            cS.check("A P^{-1} A' (KKT initialisation: A must have full row rank)", "", &f);
            // u = P^{-1} q ; t = b + A u ; y = -Schur^{-1} t
            HIPC(hipMemcpyAsync(tt, q, sizeof(T) * NP, hipMemcpyDeviceToDevice, st));
            cP.sweeps(nbP, tt, yv, xx, sw_part);
            gemv_rows<T>(st, Aonly, NP, xx, w, g, T(1), T(1), 0, MEP, 0, NP, 0);                    // w = A u + b  (padding rows: 0 + g? g holds d there)
            HIPC(hipMemsetAsync(w + me, 0, sizeof(T) * (size_t)(MEP - me), st));
            cS.sweeps(nb2, w, di, de, sw_part);                                                     // de = Schur^{-1} t
            hipLaunchKernelGGL((k_pq_scale_add<T>), g1((int)me), dim3(256), 0, st, (int)me, T(-1), de, T(0), (const T*)nullptr, dual);   // y
        }
        // x = -P^{-1}(q + A'y)
        HIPC(hipMemsetAsync(de, 0, sizeof(T) * MP, st));
        if (me > 0) HIPC(hipMemcpyAsync(de, dual, sizeof(T) * (size_t)me, hipMemcpyDeviceToDevice, st));
        const int tiles = gemv_cols_partial<T>(st, Aonly, NP, de, nullptr, T(1), T(0), part, NP, MEP, NP);
        colsum<T>(st, part, NP, tiles, q, T(1), nullptr, T(0), tt, NP);
        cP.sweeps(nbP, tt, yv, xx, sw_part);
        hipLaunchKernelGGL((k_pq_scale_add<T>), g1(NP), dim3(256), 0, st, NP, T(-1), xx, T(0), (const T*)nullptr, x);
        // s = max(d - C x, 0), z = 0                                                               (:88-89)
        gemv_rows<T>(st, G, NP, x, v, nullptr, T(1), T(0), 0, MP, 0, NP, 0);
        hipLaunchKernelGGL((k_pq_init_s<T>), g1(mtot), dim3(256), 0, st, (int)me, mtot, g, v, dual, slack);
        HIPC(hipStreamSynchronize(st));
        have_K = false;   // KK / PI were used as scratch
    }

    void solve(const qps_proxqp_params& p, qps_proxqp_report* rep) override {
        HIPC(hipSetDevice(device));
        double rho = p.rho; const double sigma = p.sigma;
        int converged = 0, conv_it = p.numIterations; double resP = INFINITY, resD = INFINITY, rho_rep = p.rho;
        update_decomposition(rho, sigma);                                                           // ProxQP.jl:131
        // Fused iteration (default): one read of G per iteration -- the pass leaves the slabs of G'w for the next right-hand
        // side, so only the first iteration, the iteration after a check and a rho change form them with the two-kernel path.
        const bool fused = p.loopVariant != 1 && apass_proxqp_slabs<T>(NP, MP) > 0;
        int slabs = 0;                                                                              // > 0: part holds the slabs of G'w for the current (s, y, z)
        for (int ii = 1; ii <= p.numIterations; ++ii) {                                             // :135
            const bool check = (ii % p.numItrConv == 0);
            if (slabs == 0) {
                hipLaunchKernelGGL((k_pq_w<T>), g1(mtot), dim3(256), 0, st, (int)me, mtot, g, dual, slack, (T)rho, w);
                slabs = gemv_cols_partial<T>(st, G, NP, w, nullptr, T(1), T(0), part, NP, MP, NP);        // G'w (:213,216)
            }
            colsum<T>(st, part, NP, slabs, x, (T)sigma, q, T(-1), tt, NP);                            // :211
            chol().sweeps(nb, tt, yv, x, sw_part);                                                  // :224 (no relaxation: x = M^{-1} r)
            if (fused && !check) {
                slabs = apass_proxqp<T>(st, G, NP, NP, MP, (int)me, x, xx, slack, dual, g, (T)rho, part, NP);   // :227-249 + next :212-216
            } else {
                gemv_rows<T>(st, G, NP, x, v, nullptr, T(1), T(0), 0, MP, 0, NP, 0);                 // A x and C x (kept: the check reads v)
                hipLaunchKernelGGL((k_pq_update<T>), g1(mtot), dim3(256), 0, st, (int)me, mtot, g, v, dual, slack, (T)rho);   // :227-249
                slabs = 0;
            }
            if (check) {                                                                            // :151  CheckConvergence! :252-298
                gemv_rows<T>(st, P, NP, x, X1, nullptr, T(1), T(0), 0, NP, 0, NP, 0);                // :261
                hipLaunchKernelGGL((k_pq_split<T>), g1(MP), dim3(256), 0, st, (int)me, MP, dual, de, di);
                int t2 = gemv_cols_partial<T>(st, G, NP, de, nullptr, T(1), T(0), part, NP, MP, NP);
                colsum<T>(st, part, NP, t2, nullptr, T(0), nullptr, T(0), X2, NP);                   // A'y (:262)
                t2 = gemv_cols_partial<T>(st, G, NP, di, nullptr, T(1), T(0), part, NP, MP, NP);
                colsum<T>(st, part, NP, t2, nullptr, T(0), nullptr, T(0), X3, NP);                   // C'z (:263)
                HIPC(hipMemsetAsync(slots, 0, 16 * sizeof(unsigned long long), st));
                hipLaunchKernelGGL((k_pq_norms<T>), dim3(64), dim3(256), 0, st, (int)n, (int)me, mtot, v, g, slack, X1, X2, X3, q, slots);
                HIPC(hipMemcpyAsync(slots_host, slots, 12 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
                HIPC(hipStreamSynchronize(st));
                const CheckOutcome co = decide(slots_host, p, rho);                                 // :266-294
                const bool updated = co.updated; rho = co.rho; converged = co.converged ? 1 : 0; resP = co.resPrim; resD = co.resDual;
                if (converged) conv_it = ii;                                                        // :155-157 (no break)
                if (updated) { update_decomposition(rho, sigma); rho_rep = rho; }                   // :159-165
            }
        }
        HIPC(hipStreamSynchronize(st));
        if (rep) { rep->converged = converged; rep->iterations = conv_it; rep->rho = rho_rep; rep->sigma = sigma; rep->resPrim = resP; rep->resDual = resD; }
    }
};

// =================================================================================================================
// SparseProxQP (ProxQP.jl:71, :95-115; sparse branches :184-190, :201-206, :335-372): the second solver form on SparseMatrixCSC inputs.
//
// The reference keeps M = P + rho (A'A + C'C) + sigma I as a sparse matrix with a frozen pattern (AlignSparsePattern :351-372, diagonal
// positions :335-349), rewrites its values on a rho update (UpdateM! :184-190) and re-factorises with the pattern-reusing `cholesky!`
// (:201-206).  Here the same linear system is solved in its KKT form
//     [P + sigma I   G' ; G   -I / rho] [x ; nu] = [sigma x - q ; h - dual / rho],     G = [A; C],  h = [b ; d - s],  dual = [y ; z]
// (eliminating nu gives exactly M x = sigma x - q + G'[rho b - y ; rho (d - s) - z], CalculateRhs! :208-219) with the sparse L D L' plugin
// of the main path: ordering + symbolic factor once per handle, a rho update is numeric only -- the pattern-reusing re-factorisation --
// and G x, which the row updates (:227-249) need, comes back with the solve (z~ = z + (nu - y) / rho = G x).  G'G is never formed: the
// reduced matrix of a sparse G is much denser than [.. G'; G ..].  CheckConvergence! (:252-298) runs on the CSR SpMVs of the main path.
// The six-argument constructor's start (:95-115: [P A'; A 0] [x; y] = [-q; b]) uses a second factor, of [P A'; A -delta I], and iterative
// refinement against the unperturbed system.
// =================================================================================================================
template <typename T> struct SparseProxQpSolver : ProxQpBase {
    // destroyed in reverse: the factor of `kkt` (it works on the stream), then inside `mats` the buffers and the stream lease
    SparseMatrices<T> mats;                       // P and G = [A; C] as CSR (mats.A = G, mats.At = G'); owns the stream, the buffers, the staging buffer
    KktPlugin<T> kkt;                             // the L D L' plugin on [P + sigma I, G'; G, -I / rho]
    hipStream_t st = nullptr;
    int mtot = 0;
    T *q = nullptr, *g = nullptr, *dual = nullptr, *slack = nullptr, *hvec = nullptr, *x = nullptr, *xx = nullptr, *v = nullptr, *de = nullptr, *di = nullptr;
    T *X1 = nullptr, *X2 = nullptr, *X3 = nullptr, *r1 = nullptr, *r2 = nullptr, *dx = nullptr, *dnu = nullptr, *zero_m = nullptr;
    unsigned long long* slots = nullptr; unsigned long long* slots_host = nullptr;
    // canonical 0-based host copies of P and A for the factor of the initialisation (dropped after init_kkt / set_state)
    KktHostCsc init;

    static dim3 g1(int64_t c) { return dim3((unsigned)((std::max<int64_t>(c, 1) + 255) / 256)); }

    SparseProxQpSolver(int dev, int64_t n_, int64_t me_, int64_t mi_, const int64_t* Pcp, const int64_t* Pri, const double* Pnz, const double* qh,
                       const int64_t* Acp, const int64_t* Ari, const double* Anz, const double* bh, const int64_t* Ccp, const int64_t* Cri, const double* Cnz,
                       const double* dh, int base)
        : mats(dev, n_, me_ + mi_), kkt(mats.st, n_, me_ + mi_) {
        device = dev; n = n_; me = me_; mi = mi_; mtot = (int)(me + mi);
        st = mats.st;
        // G = [A; C] column by column (rows of C shifted by numEq), 0-based; P re-based
        std::vector<int64_t> Gcp(n + 1, 0), Gri, P0cp(n + 1), P0ri((size_t)(Pcp[n] - base));
        std::vector<double> Gnz;
        for (int64_t j = 0; j <= n; ++j) P0cp[j] = Pcp[j] - base;
        for (size_t k = 0; k < P0ri.size(); ++k) P0ri[k] = Pri[k] - base;
        for (int64_t j = 0; j < n; ++j) {
            if (me > 0) for (int64_t k = Acp[j] - base; k < Acp[j + 1] - base; ++k) { Gri.push_back(Ari[k] - base); Gnz.push_back(Anz[k]); }
            if (mi > 0) for (int64_t k = Ccp[j] - base; k < Ccp[j + 1] - base; ++k) { Gri.push_back(Cri[k] - base + me); Gnz.push_back(Cnz[k]); }
            Gcp[j + 1] = (int64_t)Gri.size();
        }
        std::vector<double> gh((size_t)std::max(mtot, 1), 0.0);
        for (int64_t i = 0; i < me; ++i) gh[i] = bh[i];
        for (int64_t i = 0; i < mi; ++i) gh[me + i] = dh[i];
        static const int64_t dummy_i[1] = {0}; static const double dummy_d[1] = {0.0};
        if (P0cp[n] > 2000000000LL || Gcp[n] > 2000000000LL) throw QpsError(QPS_ERR_BAD_DIMENSION, "more than 2^31 non-zeros");
        // canonical host copies (sorted rows, duplicates summed): they feed the CSR copies below and, at the first solve, the analysis of the L D L' plugin
        KktHostCsc& h = kkt.host;
        layout::canonical_csc(n, P0cp.data(), P0ri.empty() ? dummy_i : P0ri.data(), Pnz, 0, h.Pcp, h.Pri, h.Pnz);
        layout::canonical_csc(n, Gcp.data(), Gri.empty() ? dummy_i : Gri.data(), Gnz.empty() ? dummy_d : Gnz.data(), 0, h.Acp, h.Ari, h.Anz);
        layout::CsrHost Ph, Gh, Gth;
        try {
            Ph = layout::csc_as_transposed_csr(n, n, h.Pcp, h.Pri, h.Pnz);
            layout::csc_to_csr_pair(mtot, n, h.Acp, h.Ari, h.Anz, Gh, Gth);
        } catch (const std::length_error& ex) { throw QpsError(QPS_ERR_BAD_DIMENSION, ex.what()); }
        mats.load(Ph, Gh, Gth);
        DeviceOwner& mem = mats.mem;
        const int64_t nn = n + 64, mm = mtot + 64;
        g = mem.dalloc<T>(mm, st); dual = mem.dalloc<T>(mm, st); slack = mem.dalloc<T>(mm, st); hvec = mem.dalloc<T>(mm, st); v = mem.dalloc<T>(mm, st); de = mem.dalloc<T>(mm, st); di = mem.dalloc<T>(mm, st);
        r2 = mem.dalloc<T>(mm, st); dnu = mem.dalloc<T>(mm, st); zero_m = mem.dalloc<T>(mm, st);
        q = mem.dalloc<T>(nn, st); x = mem.dalloc<T>(nn, st); xx = mem.dalloc<T>(nn, st); X1 = mem.dalloc<T>(nn, st); X2 = mem.dalloc<T>(nn, st); X3 = mem.dalloc<T>(nn, st); r1 = mem.dalloc<T>(nn, st); dx = mem.dalloc<T>(nn, st);
        slots = mem.dalloc<unsigned long long>(16, st);
        slots_host = mats.proxqp_slots_host();
        mats.upload_vec(qh, q, n);
        mats.upload_vec(gh.data(), g, mtot);
        init.Pcp = h.Pcp; init.Pri = h.Pri; init.Pnz = h.Pnz;
        if (me > 0) layout::canonical_csc(n, Acp, Ari, Anz, base, init.Acp, init.Ari, init.Anz);
        else init.Acp.assign(n + 1, 0);
        mats.up.reset();
    }
    ~SparseProxQpSolver() override {
        (void)hipSetDevice(device);
        (void)hipStreamSynchronize(st);
    }
    void set_state(const double* xh, const double* yh, const double* zh, const double* sh) override {
        HIPC(hipSetDevice(device));
        mats.upload_vec(xh, x, n); mats.upload_vec(yh, dual, me); mats.upload_vec(zh, dual + me, mi);
        HIPC(hipMemsetAsync(slack, 0, sizeof(T) * (size_t)(mtot + 64), st));
        mats.upload_vec(sh, slack + me, mi);
    }
    void get_state(double* xh, double* yh, double* zh, double* sh) override {
        HIPC(hipSetDevice(device));
        if (xh) mats.download_vec(x, xh, n);
        if (yh) mats.download_vec(dual, yh, me);
        if (zh) mats.download_vec(dual + me, zh, mi);
        if (sh) mats.download_vec(slack + me, sh, mi);
    }

    // ProxQP.jl:95-115: [P A'; A 0] [x; y] = [-q; b], s = max(d - C x, 0), z = 0
    void init_kkt() override {
        HIPC(hipSetDevice(device));
        if (init.released()) throw QpsError(QPS_ERR_BAD_ARGUMENT, "qps_proxqp_init_kkt: the initialisation data of this handle was released (call it once, before set_state)");
        const double delta = sizeof(T) == 8 ? 1e-8 : 1e-3;
        // (literal limits: whether this second factor should follow the QPS_LDL_* variables as the plugin's does is a behaviour question, not settled here)
        std::unique_ptr<SparseLdl<T>> start = init.template make_factor<T>(st, n, me, LdlLimits{8192, 64, 4096});
        // [P + delta I, A'; A, -delta I]: quasi-definite for every positive SEMI-definite P, so a singular P with a non-singular KKT matrix -- which the
        // reference's `mK \\ vR` (an LU, ProxQP.jl:103-106) accepts -- factorises too; the refinement below runs against the UNSHIFTED system
        start->factorize(1.0 / delta, delta);
        HIPC(hipMemsetAsync(x, 0, sizeof(T) * (size_t)(n + 64), st));
        HIPC(hipMemsetAsync(dual, 0, sizeof(T) * (size_t)(mtot + 64), st));
        HIPC(hipMemsetAsync(de, 0, sizeof(T) * (size_t)(mtot + 64), st));
        // Iterative refinement against the UNSHIFTED system until the residual stops falling (at most 50 steps).  In the directions of P that A does not pin
        // a step contracts the error only by delta / (lambda + delta): with fp32's delta = 1e-3 and lambda_min(P) = 5e-4 that is 0.67 per step, which a fixed
        // count of 7 left at 6e-2 and the handle was refused although the reference's `mK \ vR` (ProxQP.jl:103-106) solves the system.  The start need not be
        // exact (ProxQP iterates from it): it is refused only when the residual stops falling above the tolerance -- a singular [P A'; A 0], on which the reference's
        // backslash fails as well: the inconsistent part of the right-hand side stays while |x| grows by ~1 / delta per step -- or turns non-finite.
        std::vector<double> hr((size_t)n), hq((size_t)n), hr2((size_t)std::max<int64_t>(me, 1), 0.0), hb((size_t)std::max<int64_t>(me, 1), 0.0);
        auto amax = [](const std::vector<double>& a_) { double m_ = 0; for (double t : a_) { if (std::isnan(t)) return (double)INFINITY; m_ = std::fmax(m_, std::fabs(t)); } return m_; };
        mats.download_vec(q, hq.data(), n);
        if (me > 0) mats.download_vec(g, hb.data(), me);
        // against the right-hand side ONLY: a singular system answers the shifted solve with |x| ~ 1 / delta, and a scale that included |x| would
        // normalise the residual it leaves behind away
        const double scale = std::fmax(1.0, std::fmax(amax(hq), amax(hb)));
        const double target = sizeof(T) == 8 ? 1e-12 : 1e-6;
        double res0 = INFINITY, best = INFINITY, res = INFINITY; int stalled = 0;
        for (int it = 0; it <= 50; ++it) {
            // residual of the UNPERTURBED system: r1 = -q - P x - A'y, r2 = b - A x (the rows of C carry zeros in `de`, so G'de = A'y)
            { SpmvEpilogue<T> e; e.a = T(-1); e.add0 = q; e.b0 = T(-1); mats.mul(mats.P, x, r1, e); }
            if (me > 0) {
                HIPC(hipMemcpyAsync(de, dual, sizeof(T) * (size_t)me, hipMemcpyDeviceToDevice, st));
                { SpmvEpilogue<T> e; e.a = T(-1); e.add0 = r1; e.b0 = T(1); mats.mul(mats.At, de, r1, e); }
                mats.mul(mats.A, x, v);
                mats.axpby(me, T(1), g, T(-1), v, r2);
            }
            mats.download_vec(r1, hr.data(), n);
            if (me > 0) mats.download_vec(r2, hr2.data(), me);
            res = std::fmax(amax(hr), amax(hr2)) / scale;
            if (it == 0) res0 = res;
            if (!std::isfinite(res)) break;
            if (res <= target || it == 50) break;
            if (res < 0.99 * best) stalled = 0; else if (++stalled >= 3) break;  // three steps without a 1 % gain: as good as this factor gets
            best = std::fmin(best, res);
            start->solve_raw(r1, r2, dx, dnu);
            mats.axpby(n, T(1), x, T(1), dx, x);
            mats.axpby(me, T(1), dual, T(1), dnu, dual);
        }
        {
            const double accept = sizeof(T) == 8 ? 1e-6 : 1e-2;
            // refused: non-finite, or a residual that has stopped falling ABOVE the tolerance -- the floor an inconsistent (singular) system leaves, |r| = the part of
            // [-q; b] outside the range; a residual that is still falling after 50 steps is an approximate start, and a start is all ProxQP needs
            if (!std::isfinite(res) || (res > accept && stalled >= 3)) {
                char bmsg[320]; snprintf(bmsg, sizeof bmsg, "qps_proxqp_init_kkt: the iterative refinement of [P A'; A 0] [x; y] = [-q; b] did not converge (relative residual %.3g after starting at %.3g): "
                                                          "the KKT matrix is singular or too ill-conditioned", res, res0);
                throw QpsError(QPS_ERR_FACTORIZATION, bmsg);
            }
        }
        if (mtot > 0) {
            mats.mul(mats.A, x, v);                                                                 // G x
            hipLaunchKernelGGL((pqrows::k_pq_init_s<T>), g1(mtot), dim3(256), 0, st, (int)me, mtot, g, v, dual, slack);   // :110-111
        }
        HIPC(hipStreamSynchronize(st));
        init.release();
    }

    void solve(const qps_proxqp_params& p, qps_proxqp_report* rep) override {
        HIPC(hipSetDevice(device));
        init.release();
        double rho = p.rho; const double sigma = p.sigma;
        int converged = 0, conv_it = p.numIterations; double resP = INFINITY, resD = INFINITY, rho_rep = p.rho;
        kkt.prepare(rho, sigma, true);                                                              // UpdateDecomposition! (ProxQP.jl:131, :201-206)
        const char* gxs = getenv("QPS_PROXQP_GX_SOLVE");                                            // read per solve
        const bool gx_product = !(gxs && gxs[0] == '1');
        for (int ii = 1; ii <= p.numIterations; ++ii) {                                             // :135
            const bool check = (ii % p.numItrConv == 0);
            if (mtot > 0) hipLaunchKernelGGL((pqrows::k_pq_h<T>), g1(mtot), dim3(256), 0, st, (int)me, mtot, g, slack, hvec);
            kkt.ldl->solve(x, q, hvec, dual, rho, sigma, xx, v);                                    // CalculateRhs! + UpdateX! (:208-225)
            std::swap(x, xx);
            // `mA * vX`, `mC * vX` of the row updates (:230-248) by the product itself, as the reference forms them -- not the G x that falls out of the KKT solve
            // (same value up to the un-refined, un-pivoted solve's error).  The reference's check (:264-266) repeats the SAME product, so `C x - d + s` with
            // s = d - C x cancels EXACTLY on rows with z = 0; a primal residual of exactly 0 sends rho to its lower clamp (:281-283), a residual of 1e-16 to
            // rho * 1e-4: with G x from the solve in the updates and from the product in the check the two runs part for good (ProxQP fuzz, seed 43, case 184).
            if (mtot > 0 && gx_product) mats.mul(mats.A, x, v);
            if (mtot > 0) hipLaunchKernelGGL((pqrows::k_pq_update<T>), g1(mtot), dim3(256), 0, st, (int)me, mtot, g, v, dual, slack, (T)rho);   // :227-249
            if (check) {                                                                            // :151  CheckConvergence! :252-298
                mats.mul(mats.P, x, X1);                                                            // :261
                HIPC(hipMemsetAsync(X2, 0, sizeof(T) * (size_t)n, st)); HIPC(hipMemsetAsync(X3, 0, sizeof(T) * (size_t)n, st));
                if (mtot > 0) {
                    hipLaunchKernelGGL((pqrows::k_pq_split<T>), g1(mtot), dim3(256), 0, st, (int)me, mtot, dual, de, di);
                    mats.mul(mats.At, de, X2);                                                      // A'y (:262)
                    mats.mul(mats.At, di, X3);                                                      // C'z (:263)
                }
                // mA * vX, mC * vX of CheckConvergence! (:264-265): the product the row updates have just used (QPS_PROXQP_GX_SOLVE=1: recomputed here -- the
                // solve's G x carries the error of the un-refined L D L' solve, which must not go into the reported primal residual)
                if (mtot > 0 && !gx_product) mats.mul(mats.A, x, v);
                HIPC(hipMemsetAsync(slots, 0, 16 * sizeof(unsigned long long), st));
                hipLaunchKernelGGL((pqrows::k_pq_norms<T>), dim3(64), dim3(256), 0, st, (int)n, (int)me, mtot, v, g, slack, X1, X2, X3, q, slots);
                HIPC(hipMemcpyAsync(slots_host, slots, 12 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
                HIPC(hipStreamSynchronize(st));
                const pqrows::CheckOutcome co = pqrows::decide(slots_host, p, rho);                 // :266-294
                rho = co.rho; converged = co.converged ? 1 : 0; resP = co.resPrim; resD = co.resDual;
                if (converged) conv_it = ii;                                                        // :155-157 (no break)
                if (co.updated) { kkt.prepare(rho, sigma, true); rho_rep = rho; }                   // :159-165: UpdateM! + pattern-reusing cholesky!
            }
        }
        HIPC(hipStreamSynchronize(st));
        if (rep) { rep->converged = converged; rep->iterations = conv_it; rep->rho = rho_rep; rep->sigma = sigma; rep->resPrim = resP; rep->resDual = resD; }
    }
};

}  // namespace

ProxQpBase* make_proxqp(int device, int64_t n, int64_t me, int64_t mi, int dtype, const double* P, int64_t ldp, const double* A, int64_t lda,
                        const double* b, const double* C, int64_t ldc, const double* d, const double* q) {
    auto make = [&](auto s) -> ProxQpBase* { s->load(P, ldp, A, lda, b, C, ldc, d, q); return s.release(); };   // a unique_ptr: a throw while loading drops the solver
    if (dtype == QPS_F64) return make(std::make_unique<ProxQpSolver<double>>(device, n, me, mi));
    return make(std::make_unique<ProxQpSolver<float>>(device, n, me, mi));
}

ProxQpBase* make_proxqp_sparse(int device, int64_t n, int64_t me, int64_t mi, int dtype, const int64_t* Pcp, const int64_t* Pri, const double* Pnz, const double* q,
                               const int64_t* Acp, const int64_t* Ari, const double* Anz, const double* b, const int64_t* Ccp, const int64_t* Cri, const double* Cnz,
                               const double* d, int index_base) {
    if (dtype == QPS_F64) return new SparseProxQpSolver<double>(device, n, me, mi, Pcp, Pri, Pnz, q, Acp, Ari, Anz, b, Ccp, Cri, Cnz, d, index_base);
    return new SparseProxQpSolver<float>(device, n, me, mi, Pcp, Pri, Pnz, q, Acp, Ari, Anz, b, Ccp, Cri, Cnz, d, index_base);
}

}  // namespace qps
