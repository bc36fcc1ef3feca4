// dense_whitened.h -- WhitenedState: what the whitened two-launch iteration (k_pass_w.hip) of a dense fp64 handle keeps beside the classic loop's buffers.
//
// B = A W', G = W W' and the loop's vectors live in a block of their own, allocated and built at the first qualifying solve of a factor.  The loop itself is
// DenseSolver<double>::loop_whitened (qps_dense.hip); an fp32 handle holds the empty NoWhitenedState.
#pragma once
#include <cstdlib>

#include "qps_internal.h"
#include "qps_kernels.h"

namespace qps {

// what the state borrows from its solver: the stream, the padded sizes, A, the sweep matrix (S lower = W: one inverted block) and the factorisation's scratch
template <typename T> struct WhitenedView { hipStream_t st; int NP, MP; const T *A, *S; T* tmp; };

struct WhitenedState {
    Arena arena;
    double *B = nullptr, *G = nullptr, *slab_e = nullptr, *slab_g = nullptr, *slab_y = nullptr;
    double *u = nullptr, *p0 = nullptr, *p1 = nullptr, *c = nullptr, *gd = nullptr, *bty = nullptr, *a = nullptr;
    int mode = -1; bool valid = false, failed = false;
    int cat_pass = 0, cat_passchk = 0, cat_sum = 0, cat_l = 0;
    // QPS_WHITEN, read when the handle is created: 0 never, 1 wherever supported, unset: 2048 < NP <= 4096
    WhitenedState() { const char* e = getenv("QPS_WHITEN"); mode = e ? atoi(e) : -1; }
    // the stacked matrix [B ; tril(G)] once + u, gd, z, y, a, l, u in / out; the slab sum reads two slab sets
    void categories(Profiler& prof, double n, double m) {
        const double s = sizeof(double);
        cat_pass = prof.category("apass(fused A-pass; whitened, stacked with G)", s * (m * n + n * (n + 1) / 2 + 2.0 * n + 8.0 * m));
        cat_passchk = prof.category("apass(check variant; whitened)", s * (m * n + n * (n + 1) / 2 + 2.0 * n + 8.0 * m));
        cat_sum = prof.category("wsum(whitened slab sums: p+, u+)", s * (2.0 * whitened_slabs() * n + 5.0 * n));
        cat_l = prof.category("lpass(x, x - xp, A'y: triangle of L once)", s * (n * (n + 1) / 2 + 5.0 * n));
    }
    void invalidate() { valid = false; }   // a new factor: B and G are rebuilt at its first qualifying solve
    bool wanted(int NP) const { return mode == 1 || (mode < 0 && NP > 2048 && NP <= 4096); }   // auto: the measured band (eager classic loop, four chunks per thread)
    // B and G of the current factor.  false: the block could not be allocated, the handle stays on the classic loop for good.
    bool build(const WhitenedView<double>& v) {
        if (valid) return true;
        if (failed) return false;
        if (!B) {
            auto layout = [&] {
                const int64_t sl = (int64_t)whitened_slabs() * v.NP;
                B = arena.take<double>((int64_t)v.MP * v.NP); G = arena.take<double>((int64_t)v.NP * v.NP);
                slab_e = arena.take<double>(sl); slab_g = arena.take<double>(sl); slab_y = arena.take<double>(sl);
                u = arena.take<double>(v.NP); p0 = arena.take<double>(v.NP); p1 = arena.take<double>(v.NP); c = arena.take<double>(v.NP);
                gd = arena.take<double>(v.NP); bty = arena.take<double>(v.NP); a = arena.take<double>(v.MP);
            };
            layout();
            if (!arena.try_commit(v.st)) { failed = true; return false; }
            layout();
        }
        tril_copy(v.st, v.S, v.tmp, v.NP);                                                                    // W with zeros above the diagonal (tmp: free after factor())
        gemm<double>(v.st, v.MP, v.NP, v.NP, 1.0, v.A, v.NP, true, v.tmp, v.NP, true, 0.0, B, v.NP, false, 1, 0, 0, 0, 4);     // B[i][j] = sum_{k <= j} A[i][k] W[j][k]
        gemm<double>(v.st, v.NP, v.NP, v.NP, 1.0, v.tmp, v.NP, true, v.tmp, v.NP, true, 0.0, G, v.NP, true, 1, 0, 0, 0, 4);    // G[i][j] = sum_{k <= j} W[i][k] W[j][k], j <= i
        valid = true;
        return true;
    }
    // the argument blocks of the two loop kernels; the pass reads u and leaves gd and the three slab sets, the sum turns them into p_new and the next u
    WhitenedPass<double> pass_args(const WhitenedView<double>& v, double* z, double* y, const double* l, const double* hi, double alpha, double rho,
                                   unsigned long long* slots) const {
        WhitenedPass<double> w;
        w.B = B; w.G = G; w.ld = v.NP; w.NP = v.NP; w.MP = v.MP; w.u = u; w.z = z; w.y = y; w.a = a; w.l = l; w.hi = hi;
        w.alpha = alpha; w.rho = rho; w.gd = gd; w.slab_e = slab_e; w.slab_g = slab_g; w.slab_y = slab_y; w.part_ld = v.NP; w.slots = slots;
        return w;
    }
    WhitenedSum<double> sum_args(int NP, bool first, const double* p_old, double* p_new, double alpha, double sigma) const {
        WhitenedSum<double> w;
        w.slab_e = slab_e; w.slab_g = slab_g; w.slab_y = slab_y; w.part_ld = NP; w.ntiles = whitened_slabs(); w.ncols = NP; w.first = first;
        w.gd = gd; w.p_old = p_old; w.c = c; w.p_new = p_new; w.u = u; w.bty = bty; w.alpha = alpha; w.sigma = sigma;
        return w;
    }
};
// fp32 handles: the route is never chosen, nothing is held
struct NoWhitenedState {
    void categories(Profiler&, double, double) {}
    void invalidate() {}
    bool wanted(int) const { return false; }
    template <typename V> bool build(const V&) { return false; }
};

}  // namespace qps
