// dense_chol.h -- the factor-and-sweep path of the dense solvers (DenseSolver, BatchedDenseSolver in qps_capi.hip; ProxQpSolver in qps_proxqp.hip):
// M = P + sigma I + rho G'G (LinearSystemSolvers.jl:112-114 / :127-129, ProxQP.jl:175-181), its Cholesky factor turned into the sweep matrix S
// (qps_kernels.h), the breakdown check, and x = (L L')^{-1} r by the two triangular sweeps over S.  It works on buffers its caller owns.
#pragma once
#include <cstdlib>
#include <vector>

#include "qps_internal.h"
#include "qps_kernels.h"

namespace qps {

// Diagonal block size of the sweep matrix: one inverted block over the whole factor while the fused forward+backward sweep covers NP, else 4096;
// a request (> 0) is rounded down to a power-of-two multiple of 64.  Halved while half of it still covers NP.
template <typename T> inline int pick_nb(int requested, int NP) {
    int nb = requested > 0 ? requested : (sweep_fused_supported<T>(NP) ? 32768 : 4096);
    int p = 64; while (p * 2 <= nb) p *= 2;
    nb = p;
    while (nb > 64 && nb / 2 >= NP) nb /= 2;
    return nb;
}

// qps_info.sweepVariant of DenseChol::sweeps: 2 = fused pass over one block, 3 = two sweeps over one block, 1 = one launch per block phase.
// QPS_SWEEP_MODE=0 (read once per process) turns the fused pass off.
template <typename T> inline int chol_sweep_variant(int NP, int nb) {
    static const int mode = getenv("QPS_SWEEP_MODE") ? atoi(getenv("QPS_SWEEP_MODE")) : 2;
    if (nb < NP) return 1;
    return (mode == 2 && sweep_fused_supported<T>(NP)) ? 2 : 3;
}

// Profiler brackets of the sweeps, as data; a category of -1 is not bracketed.  The fused pass and the column sum of its slabs are timed per
// dispatch (ProfLaunchScope at fused_lvl / xsum_lvl), the forward and the backward block-phase sweep as one run of launches each (ProfScope at run_lvl).
struct SweepProf { Profiler* prof = nullptr; int fused = -1, fused_lvl = 0, xsum = -1, xsum_lvl = 0, fwd = -1, bwd = -1, run_lvl = 0; };

// `count` systems back to back: P, PI, GG, M, S, tmp NP*NP apart, G (row-major, ld NP) MP*NP apart, dinv (NP/64)*4096 apart, fail 1 apart.
template <typename T> struct DenseChol {
    hipStream_t st = nullptr;
    int n = 0, NP = 0, MP = 0;   // order of P, padded order of M, padded rows of G
    const T *P = nullptr, *G = nullptr;
    T *PI = nullptr, *GG = nullptr, *M = nullptr, *S = nullptr, *tmp = nullptr, *dinv = nullptr; int* fail = nullptr;

    DenseChol at(int b) const {   // system b alone
        const int64_t nn = (int64_t)NP * NP;
        DenseChol c = *this;
        c.P = P + b * nn; c.G = G + b * (int64_t)MP * NP; c.PI = PI + b * nn; c.GG = GG + b * nn; c.M = M + b * nn; c.S = S + b * nn; c.tmp = tmp + b * nn;
        c.dinv = dinv + b * (int64_t)(NP / 64) * 4096; c.fail = fail + b;
        return c;
    }
    // M = PI + rho GG, after PI = P + sigma I (pi) and GG = G'G (gg) when the caller says they are stale; rho_arr: per-system rho (device)
    void form(double sigma, double rho, bool pi, bool gg, int count = 1, const double* rho_arr = nullptr) const {
        const int64_t nn = (int64_t)NP * NP;
        if (pi) make_PI<T>(st, n, NP, P, (T)sigma, PI, count);
        if (gg && MP > 0) {
            const int64_t sG = count > 1 ? (int64_t)MP * NP : 0, sC = count > 1 ? nn : 0;
            gemm<T>(st, NP, NP, MP, T(1), G, NP, false, G, NP, false, T(0), GG, NP, true, count, sG, sG, sC);
        } else if (gg) HIPC(hipMemsetAsync(GG, 0, sizeof(T) * (size_t)(count * nn), st));
        assemble_M<T>(st, NP, PI, GG, (T)rho, M, count, rho_arr);
    }
    // Cholesky of M in place (S is rebuilt right after: free as its scratch), then the sweep matrix S (premul: the blocked sweeps' form)
    void factor(int nb, int count = 1, bool premul = false) const {
        cholesky<T>(st, NP, M, dinv, fail, count, chol_scratch_fits(NP) ? S : nullptr);
        build_sweep_matrix<T>(st, NP, nb, M, dinv, S, tmp, count, premul);
    }
    // Reads back the fail words of `count` systems into `host` and throws QPS_ERR_FACTORIZATION for the first that broke down among the QPs
    // `batch` lists (its message names the QP), or for system 0 when batch is null.  what: the caller's name of M; ctx: appended in parentheses.
    void check(const char* what, const char* ctx, int* host, int count = 1, const std::vector<int>* batch = nullptr) const {
        if (batch && batch->empty()) return;
        HIPC(hipMemcpyAsync(host, fail, sizeof(int) * count, hipMemcpyDeviceToHost, st));
        HIPC(hipStreamSynchronize(st));
        for (size_t k = 0; k < (batch ? batch->size() : 1); ++k) {
            const int b = batch ? (*batch)[k] : 0, f = host[b];
            if (f == 0) continue;
            char pre[64] = "", msg[512];
            if (batch) snprintf(pre, sizeof pre, "QP %d of the batch: ", b);
            if (f > 0) snprintf(msg, sizeof msg, "%sCholesky of %s broke down: non-positive pivot at column %d%s%s%s", pre, what, f, *ctx ? " (" : "", ctx, *ctx ? ")" : "");
            else snprintf(msg, sizeof msg, "%sCholesky of %s: the diagonal workgroup of a fused update launch gave up waiting for its two tiles (k_chol_update_diag%s%s)",
                          pre, what, *ctx ? "; " : "", ctx);
            throw QpsError(QPS_ERR_FACTORIZATION, msg);
        }
    }
    // x = (L L')^{-1} r over S with nb x nb diagonal blocks, for bs.count systems (BatchStride(): one).  r is consumed, y is work space, part receives
    // the fused pass's slabs (sweep_fused_slabs<T>(NP, bs.count) * NP per system).
    void sweeps(int nb, T* r, T* y, T* x, T* part, BatchStride bs = BatchStride(), const SweepProf& pf = SweepProf()) const {
        if (chol_sweep_variant<T>(NP, nb) == 2) {
            // one inverted block: forward and backward sweep read the same entries -> one fused pass over the triangle, then the sum of its slabs
            BatchStride bw = bs, bx = bs;
            bw.vout = bx.mat = bs.count > 1 ? (int64_t)sweep_fused_slabs<T>(NP, bs.count) * NP : 0;   // slab sets of a batch
            int Gs = 0;
            bracket_launch(pf.prof, pf.fused, pf.fused_lvl, [&] { Gs = sweep_fused<T>(st, S, NP, NP, r, part, NP, bw); });
            bracket_launch(pf.prof, pf.xsum, pf.xsum_lvl, [&] { colsum<T>(st, part, NP, Gs, nullptr, T(0), nullptr, T(0), x, NP, bx); });
            return;
        }
        const int nblk = (NP + nb - 1) / nb;
        bracket_run(pf.prof, pf.fwd, pf.run_lvl, [&] {
            for (int J = 0; J < nblk; ++J) {
                const int r0 = J * nb, r1 = std::min(NP, r0 + nb);
                gemv_rows<T>(st, S, NP, r, y, nullptr, T(1), T(0), r0, r1, r0, r1, 1, bs);
                if (r1 < NP) gemv_rows<T>(st, S, NP, y, r, r, T(-1), T(1), r1, NP, r0, r1, 0, bs);
            }
        });
        bracket_run(pf.prof, pf.bwd, pf.run_lvl, [&] {
            for (int J = nblk - 1; J >= 0; --J) {
                const int r0 = J * nb, r1 = std::min(NP, r0 + nb);
                gemv_rows<T>(st, S, NP, y, x, nullptr, T(1), T(0), r0, r1, r0, r1, 2, bs);
                if (r0 > 0) gemv_rows<T>(st, S, NP, x, y, y, T(-1), T(1), 0, r0, r0, r1, 0, bs);
            }
        });
    }

    template <typename F> static void bracket_launch(Profiler* p, int cat, int lvl, F&& f) { if (p && cat >= 0) { ProfLaunchScope s(*p, cat, lvl); f(); } else f(); }
    template <typename F> static void bracket_run(Profiler* p, int cat, int lvl, F&& f) { if (p && cat >= 0) { ProfScope s(*p, cat, lvl); f(); } else f(); }
};

}  // namespace qps
