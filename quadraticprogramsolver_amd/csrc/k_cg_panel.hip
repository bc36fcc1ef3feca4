// k_cg_panel.hip -- the matrix-free CG plugin (LinOpCg!, LinearSystemSolvers.jl:145-186) of the shared-matrix batches: one cg! per column, all columns of a
// batch in lockstep on 16-column panels [panel][rows][16].
//
// The products are the strip kernels of panel_strips.h (one (matrix row, panel) per 16 SPR lanes, blockIdx.y = panel, fixed summation order); the vector kernels
// give one thread one (row, column).  A workgroup takes `reps` consecutive row groups, so that a launch has a bounded number of workgroups per panel:
// every dot product is one double partial per (workgroup, column), [panel][workgroup][16], and every consumer adds the partials of its column in workgroup
// order -- the same sum in every workgroup, a function of the matrices' shape alone, never of the batch around the column.  The CG scalars of a column live in
// CgPanelState, ping-ponged between the two halves of `state` by k_cgp_next_u.  No atomics, no grid barrier, nothing waits on another workgroup.
//
// A column that is done (converged, at its iteration limit, or not active in the ADMM loop) keeps x~, r, u and its scalars: every store to them is skipped.
#include <algorithm>
#include <type_traits>

#include "panel_strips.h"
#include "qps_kernels.h"

namespace qps {

namespace {

// Workgroups per panel of a launch that writes partials.  The operator wants many (a row group is a chain of dependent gathers: occupancy hides it), the vector
// kernels few: each of their workgroups reads every partial of its 16 columns, 128 bytes per producer workgroup.
constexpr int CGP_MAX_OP_BLOCKS = 2048, CGP_MAX_VEC_BLOCKS = 256;

inline int cgp_groups(int rows, int rpb) { return (rows + rpb - 1) / rpb; }
inline int cgp_reps(int rows, int rpb, int cap) { return std::max(1, (cgp_groups(rows, rpb) + cap - 1) / cap); }
inline int cgp_blocks(int rows, int rpb, int cap) { const int r = cgp_reps(rows, rpb, cap); return (cgp_groups(rows, rpb) + r - 1) / r; }

// Sum of d over the 256 threads of the workgroup that share the lane's column (lane % 16), in every thread: the four DPP rows of a wave, then
// (w0 + w1) + (w2 + w3) through LDS.  Every thread of the workgroup calls it.
__device__ __forceinline__ double wg_col_sum(double d, double (*sh)[16]) {
    d += __shfl_xor(d, 16);
    d += __shfl_xor(d, 32);
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, c = threadIdx.x & 15;
    __syncthreads();   // the previous user of sh is done with it
    if (lane < 16) sh[w][lane] = d;
    __syncthreads();
    return (sh[0][c] + sh[1][c]) + (sh[2][c] + sh[3][c]);
}
// Sum of the nblk partials of the lane's column (part: [nblk][16] of this panel), in every thread: 16 interleaved chains, then those in order.
__device__ __forceinline__ double part_col_sum(const double* __restrict__ part, int nblk, double (*sh)[16]) {
    const int g = threadIdx.x >> 4, c = threadIdx.x & 15;
    double s = 0.0;
    for (int b = g; b < nblk; b += 16) s += part[(int64_t)b * 16 + c];
    __syncthreads();
    sh[g][c] = s;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < 16; ++k) t += sh[k][c];
    return t;
}
// one more CG iteration's ||r||^2 folded into the scalars of a column that is still running (the tail of cg!'s loop body)
__device__ __forceinline__ void cgp_fold(CgPanelState& s, double rr, int maxit) {
    if (s.done) return;
    s.prev2 = s.res2; s.res2 = rr; s.itn += 1;
    if (sqrt(rr) <= s.tol || s.itn >= maxit) s.done = 1;
}

// t = sigma x - q + A'w (LinearSystemSolvers.jl:177-178); w = rho_i z - y comes from panel_w
template <typename T, int SPR>
__global__ __launch_bounds__(PS_THREADS) void k_cgp_rhs(int n, int m, const int* __restrict__ rp, const int* __restrict__ ci, const T* __restrict__ va,
                                                         const T* __restrict__ w, const T* __restrict__ x, const T* __restrict__ q, T sigma, T* __restrict__ t) {
    const int r = blockIdx.x * (PS_THREADS / (16 * SPR)) + threadIdx.x / (16 * SPR), strip = (threadIdx.x >> 4) % SPR, col = threadIdx.x & 15;
    const bool valid = r < n;
    const T* wp = w + (int64_t)blockIdx.y * m * 16 + col;
    T s = T(0);
    if (valid) s = strip_dot<T, SPR>(rp[r], rp[r + 1], strip, ci, va, [&](int i) { return wp[(int64_t)i * 16]; });
    s = strips_sum<T, SPR>(s);
    if (valid && strip == 0) { const int64_t i = ((int64_t)blockIdx.y * n + r) * 16 + col; t[i] = sigma * x[i] - q[i] + s; }
}

// rho of (row r, column c of the batch) under qps_set_shared_column_rho: rho_b, times s_i where a row scale is set (rho_row then holds s_i: two roundings)
template <typename T> __device__ __forceinline__ T cgp_col_rho(T rc, const T* __restrict__ rho_row, int r) { return rho_row ? rc * rho_row[r] : rc; }

// first launch of the operator: v = rho_i (A u).  st != NULL: a panel whose columns are all done is skipped.  COL: rho_b of the thread's column from rho_col --
// the 16 values of a panel are one line, loaded once per thread before the strips
template <typename T, int SPR, bool COL>
__global__ __launch_bounds__(PS_THREADS) void k_cgp_av(int m, int n, const int* __restrict__ rp, const int* __restrict__ ci, const T* __restrict__ va,
                                                        const T* __restrict__ u, const T* __restrict__ rho_row, T rho, const T* __restrict__ rho_col,
                                                        const CgPanelState* __restrict__ st, T* __restrict__ v) {
    const int r = blockIdx.x * (PS_THREADS / (16 * SPR)) + threadIdx.x / (16 * SPR), strip = (threadIdx.x >> 4) % SPR, col = threadIdx.x & 15;
    if (st && __syncthreads_and(st[blockIdx.y * 16 + col].done)) return;
    const bool valid = r < m;
    const T* up = u + (int64_t)blockIdx.y * n * 16 + col;
    T rc = rho;
    if (COL) rc = rho_col[blockIdx.y * 16 + col];
    T s = T(0);
    if (valid) s = strip_dot<T, SPR>(rp[r], rp[r + 1], strip, ci, va, [&](int i) { return up[(int64_t)i * 16]; });
    s = strips_sum<T, SPR>(s);
    if (valid && strip == 0) v[((int64_t)blockIdx.y * m + r) * 16 + col] = (COL ? cgp_col_rho(rc, rho_row, r) : (rho_row ? rho_row[r] : rho)) * s;
}

// second launch of the operator: row r of P over u, then row r of A' over v, c_r = that + sigma u_r (LinearSystemSolvers.jl:152-157).
// INIT = 0: c is stored and part takes the workgroup's share of u'c.  INIT = 1 (u = x~): r = t - c, u = 0 on the active columns and part takes ||r||^2.
template <typename T, int SPR, int INIT>
__global__ __launch_bounds__(PS_THREADS) void k_cgp_op(int n, int m, int reps, const int* __restrict__ Prp, const int* __restrict__ Pci, const T* __restrict__ Pva,
                                                        const int* __restrict__ Arp, const int* __restrict__ Aci, const T* __restrict__ Ava,
                                                        const T* __restrict__ u, const T* __restrict__ v, T sigma, const T* __restrict__ t,
                                                        const int* __restrict__ active, const CgPanelState* __restrict__ st, T* __restrict__ c,
                                                        T* __restrict__ rvec, T* __restrict__ unew, double* __restrict__ part) {
    constexpr int RPB = PS_THREADS / (16 * SPR);
    __shared__ double sh[4][16];
    const int P = blockIdx.y, strip = (threadIdx.x >> 4) % SPR, col = threadIdx.x & 15;
    if (!INIT && __syncthreads_and(st[P * 16 + col].done)) return;
    const T* up = u + (int64_t)P * n * 16 + col;
    const T* vp = v + (int64_t)P * m * 16 + col;
    const bool store = INIT ? active[P * 16 + col] != 0 : true;
    double acc = 0.0;
    for (int k = 0; k < reps; ++k) {
        const int64_t r = ((int64_t)blockIdx.x * reps + k) * RPB + threadIdx.x / (16 * SPR);
        const bool valid = r < n;
        T s = T(0);
        if (valid) {
            s = strip_dot<T, SPR>(Prp[r], Prp[r + 1], strip, Pci, Pva, [&](int i) { return up[(int64_t)i * 16]; });
            s += strip_dot<T, SPR>(Arp[r], Arp[r + 1], strip, Aci, Ava, [&](int i) { return vp[(int64_t)i * 16]; });
        }
        s = strips_sum<T, SPR>(s);
        if (valid && strip == 0) {
            const int64_t i = ((int64_t)P * n + r) * 16 + col;
            const T ur = up[r * 16];
            const T cr = s + sigma * ur;
            if (INIT) {
                const T ri = t[i] - cr;
                if (store) { rvec[i] = ri; unew[i] = T(0); }
                acc += (double)ri * (double)ri;
            } else {
                c[i] = cr;
                acc += (double)ur * (double)cr;
            }
        }
        if (SPR == 16) __syncthreads();   // strips_sum's LDS is written again in the next round
    }
    acc = wg_col_sum(acc, sh);
    if (threadIdx.x < 16) part[((int64_t)P * gridDim.x + blockIdx.x) * 16 + threadIdx.x] = acc;
}

// cg!'s start: tol = max(sqrt(eps(T)) ||r0||, epsPcg); a column is born done when it is inactive or already within tol.  One workgroup per panel.
__global__ __launch_bounds__(256) void k_cgp_init_final(const double* __restrict__ part, int nblk, const int* __restrict__ active, double abstol, double reltol,
                                                        CgPanelState* __restrict__ st) {
    __shared__ double sh[16][16];
    const double d = part_col_sum(part + (int64_t)blockIdx.x * nblk * 16, nblk, sh);
    if (threadIdx.x < 16) {
        const int b = blockIdx.x * 16 + threadIdx.x;
        const double residual = sqrt(d);
        CgPanelState s;
        s.res2 = d; s.prev2 = 1.0; s.tol = fmax(reltol * residual, abstol); s.itn = 0;
        s.done = (!active[b] || residual <= s.tol) ? 1 : 0;
        st[b] = s;
    }
}

// Head of a CG iteration: the ||r||^2 partials of the previous one are folded (first = 1: the scalars are current already), block 0 of a panel writes the
// OTHER half of the state, then u = r + beta u with beta = res2 / prev2 (prev2 = 1 and u = 0 at the first iteration: u = r).
template <typename T>
__global__ __launch_bounds__(256) void k_cgp_next_u(int n, int reps, const double* __restrict__ part_rr, const T* __restrict__ r, T* __restrict__ u,
                                                    const CgPanelState* __restrict__ cur, CgPanelState* __restrict__ nxt, int first, int maxit) {
    __shared__ double sh[16][16];
    const int P = blockIdx.y, col = threadIdx.x & 15;
    CgPanelState s = cur[P * 16 + col];
    if (!first) {
        const double rr = part_col_sum(part_rr + (int64_t)P * gridDim.x * 16, (int)gridDim.x, sh);
        cgp_fold(s, rr, maxit);
    }
    if (blockIdx.x == 0 && threadIdx.x < 16) nxt[P * 16 + col] = s;
    if (s.done) return;
    const T beta = (T)(s.res2 / s.prev2);
    for (int k = 0; k < reps; ++k) {
        const int64_t row = ((int64_t)blockIdx.x * reps + k) * 16 + (threadIdx.x >> 4);
        if (row < n) { const int64_t i = ((int64_t)P * n + row) * 16 + col; u[i] = r[i] + beta * u[i]; }
    }
}

// alpha = res2 / u'c re-derived from the partials in every workgroup; x~ += alpha u, r -= alpha c, partials of ||r||^2
template <typename T>
__global__ __launch_bounds__(256) void k_cgp_update(int n, int reps, const double* __restrict__ part_uc, int nblk_uc, const T* __restrict__ u,
                                                    const T* __restrict__ c, T* __restrict__ xx, T* __restrict__ r, double* __restrict__ part_rr,
                                                    const CgPanelState* __restrict__ st) {
    __shared__ double sh[16][16];
    const int P = blockIdx.y, col = threadIdx.x & 15;
    const CgPanelState s = st[P * 16 + col];
    if (__syncthreads_and(s.done)) return;
    const double uc = part_col_sum(part_uc + (int64_t)P * nblk_uc * 16, nblk_uc, sh);
    double acc = 0.0;
    if (!s.done) {
        const T alpha = (T)(s.res2 / uc);
        for (int k = 0; k < reps; ++k) {
            const int64_t row = ((int64_t)blockIdx.x * reps + k) * 16 + (threadIdx.x >> 4);
            if (row < n) {
                const int64_t i = ((int64_t)P * n + row) * 16 + col;
                xx[i] += alpha * u[i];
                const T ri = r[i] - alpha * c[i];
                r[i] = ri;
                acc += (double)ri * (double)ri;
            }
        }
    }
    acc = wg_col_sum(acc, sh);
    if (threadIdx.x < 16) part_rr[((int64_t)P * gridDim.x + blockIdx.x) * 16 + threadIdx.x] = acc;
}

// end of a burst: the last iteration's ||r||^2 folded in place, so that the host reads current scalars.  One workgroup per panel.
__global__ __launch_bounds__(256) void k_cgp_finish(const double* __restrict__ part_rr, int nblk, CgPanelState* __restrict__ st, int maxit) {
    __shared__ double sh[16][16];
    const double rr = part_col_sum(part_rr + (int64_t)blockIdx.x * nblk * 16, nblk, sh);
    if (threadIdx.x < 16) {
        CgPanelState s = st[blockIdx.x * 16 + threadIdx.x];
        if (!s.done) { cgp_fold(s, rr, maxit); st[blockIdx.x * 16 + threadIdx.x] = s; }
    }
}

// z~ = A x~ (LinearSystemSolvers.jl:181) with the row update of SolveQuadraticProgram.jl:59-61 as its epilogue, on the active columns; rho_i where a scale is set.
// COL: rho_b and 1 / rho_b of the thread's column from rho_col / rho1_col, as in k_cgp_av
template <typename T, int SPR, bool COL>
__global__ __launch_bounds__(PS_THREADS) void k_cgp_post_rows(int m, int n, const int* __restrict__ rp, const int* __restrict__ ci, const T* __restrict__ va,
                                                              const T* __restrict__ xx, T* __restrict__ z, T* __restrict__ zp, T* __restrict__ y,
                                                              const T* __restrict__ lo, const T* __restrict__ hi, const int* __restrict__ active, T alpha, T rho,
                                                              const T* __restrict__ rho_row, const T* __restrict__ rho1_row, const T* __restrict__ rho_col,
                                                              const T* __restrict__ rho1_col) {
    const int r = blockIdx.x * (PS_THREADS / (16 * SPR)) + threadIdx.x / (16 * SPR), strip = (threadIdx.x >> 4) % SPR, col = threadIdx.x & 15;
    const bool valid = r < m;
    const T* xp = xx + (int64_t)blockIdx.y * n * 16 + col;
    T rc = rho, rc1 = T(0);
    if (COL) { rc = rho_col[blockIdx.y * 16 + col]; rc1 = rho1_col[blockIdx.y * 16 + col]; }
    T s = T(0);
    if (valid) s = strip_dot<T, SPR>(rp[r], rp[r + 1], strip, ci, va, [&](int i) { return xp[(int64_t)i * 16]; });
    s = strips_sum<T, SPR>(s);
    if (valid && strip == 0 && active[blockIdx.y * 16 + col]) {
        const int64_t i = ((int64_t)blockIdx.y * m + r) * 16 + col;
        const T rr = COL ? cgp_col_rho(rc, rho_row, r) : (rho_row ? rho_row[r] : rho);
        const T rr1 = COL ? cgp_col_rho(rc1, rho1_row, r) : (rho_row ? rho1_row[r] : T(1) / rho), alpha1 = T(1) - alpha;
        const T zo = z[i], yo = y[i];
        zp[i] = zo;                                                           // :59
        const T t = alpha * s + alpha1 * zo + rr1 * yo;                       // :60
        const T l = lo[i], h = hi[i];
        const T zn = t > h ? h : (t < l ? l : t);
        z[i] = zn;
        y[i] = yo + rr * (alpha * s + alpha1 * zo - zn);                      // :61
    }
}
// xp = x; x = alpha x~ + (1 - alpha) x on the active columns (SolveQuadraticProgram.jl:56-57)
template <typename T>
__global__ __launch_bounds__(256) void k_cgp_post_x(int64_t per_panel, int64_t total, const T* __restrict__ xx, T* __restrict__ x, T* __restrict__ xp,
                                                    const int* __restrict__ active, T alpha) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    if (!active[(int)(i / per_panel) * 16 + (int)(i & 15)]) return;
    const T xo = x[i];
    xp[i] = xo;
    x[i] = alpha * xx[i] + (T(1) - alpha) * xo;
}

// w = rho_b z - y on the active columns under qps_set_shared_column_rho (LinearSystemSolvers.jl:176): the expression of panel_w with the column's own rho, one
// thread per (row, column); a stopped column keeps its w
template <typename T>
__global__ __launch_bounds__(256) void k_cgp_w(int64_t per_panel, int64_t total, const T* __restrict__ z, const T* __restrict__ y, const int* __restrict__ active,
                                               const T* __restrict__ rho_row, const T* __restrict__ rho_col, T* __restrict__ w) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i / per_panel) * 16 + (int)(i & 15);
    if (!active[c]) return;
    const T rr = cgp_col_rho(rho_col[c], rho_row, (int)((i % per_panel) >> 4));
    w[i] = rr * z[i] - y[i];
}

template <int SPR> constexpr int rpb_of() { return PS_THREADS / (16 * SPR); }

// F(std::integral_constant<int, SPR>) for the strip count spr
template <typename F> inline void with_spr(int spr, F&& f) {
    if (spr == 1) f(std::integral_constant<int, 1>());
    else if (spr == 4) f(std::integral_constant<int, 4>());
    else f(std::integral_constant<int, 16>());
}

template <typename T, int INIT>
void cgp_operator(hipStream_t st, const CgPanelArgs<T>& a, const T* u, const CgPanelState* state) {
    with_spr(a.A.spr, [&](auto S) {
        constexpr int SPR = decltype(S)::value;
        const dim3 grid((unsigned)cgp_groups(a.m, rpb_of<SPR>()), (unsigned)a.npanel);
        if (a.rho_col) hipLaunchKernelGGL((k_cgp_av<T, SPR, true>), grid, dim3(PS_THREADS), 0, st, a.m, a.n, a.A.rp, a.A.ci, a.A.va, u, a.rho_row, a.rho, a.rho_col,
                                          INIT ? nullptr : state, a.v);
        else hipLaunchKernelGGL((k_cgp_av<T, SPR, false>), grid, dim3(PS_THREADS), 0, st, a.m, a.n, a.A.rp, a.A.ci, a.A.va, u, a.rho_row, a.rho, a.rho_col,
                                INIT ? nullptr : state, a.v);
    });
    with_spr(a.spr_op, [&](auto S) {
        constexpr int SPR = decltype(S)::value;
        const int rpb = rpb_of<SPR>();
        hipLaunchKernelGGL((k_cgp_op<T, SPR, INIT>), dim3((unsigned)cgp_blocks(a.n, rpb, CGP_MAX_OP_BLOCKS), (unsigned)a.npanel), dim3(PS_THREADS), 0, st, a.n, a.m, cgp_reps(a.n, rpb, CGP_MAX_OP_BLOCKS),
                           a.P.rp, a.P.ci, a.P.va, a.At.rp, a.At.ci, a.At.va, u, (const T*)a.v, a.sigma, (const T*)a.t, a.active, state, a.c, a.r, a.u, a.part_uc);
    });
}

}  // namespace

int cg_panel_op_spr(int64_t nnzP, int64_t nnzA, int n) { return pick_panel_spr(nnzP + nnzA, n); }
int cg_panel_op_blocks(int rows, int spr) { return cgp_blocks(rows, PS_THREADS / (16 * spr), CGP_MAX_OP_BLOCKS); }
int cg_panel_vec_blocks(int rows) { return cgp_blocks(rows, 16, CGP_MAX_VEC_BLOCKS); }

template <typename T> void cg_panel_begin(hipStream_t st, const CgPanelArgs<T>& a) {
    if (a.n <= 0 || a.m <= 0 || a.npanel <= 0) return;
    with_spr(a.At.spr, [&](auto S) {
        constexpr int SPR = decltype(S)::value;
        hipLaunchKernelGGL((k_cgp_rhs<T, SPR>), dim3((unsigned)cgp_groups(a.n, rpb_of<SPR>()), (unsigned)a.npanel), dim3(PS_THREADS), 0, st, a.n, a.m, a.At.rp, a.At.ci,
                           a.At.va, a.w, a.x, a.q, a.sigma, a.t);
    });
    cgp_operator<T, 1>(st, a, a.xx, nullptr);
    hipLaunchKernelGGL(k_cgp_init_final, dim3((unsigned)a.npanel), dim3(256), 0, st, (const double*)a.part_uc, cg_panel_op_blocks(a.n, a.spr_op), a.active, a.eps_pcg,
                       sizeof(T) == 8 ? 1.4901161193847656e-08 : 3.4526698300124393e-04, a.state);
}

template <typename T> void cg_panel_iteration(hipStream_t st, const CgPanelArgs<T>& a, int cur, bool first) {
    if (a.n <= 0 || a.m <= 0 || a.npanel <= 0) return;
    const int CP = 16 * a.npanel, nbv = cg_panel_vec_blocks(a.n), rv = cgp_reps(a.n, 16, CGP_MAX_VEC_BLOCKS);
    const CgPanelState* sc = a.state + (int64_t)cur * CP;
    CgPanelState* sn = a.state + (int64_t)(cur ^ 1) * CP;
    hipLaunchKernelGGL((k_cgp_next_u<T>), dim3((unsigned)nbv, (unsigned)a.npanel), dim3(256), 0, st, a.n, rv, (const double*)a.part_rr, (const T*)a.r, a.u, sc, sn,
                       first ? 1 : 0, a.max_it);
    cgp_operator<T, 0>(st, a, a.u, sn);
    hipLaunchKernelGGL((k_cgp_update<T>), dim3((unsigned)nbv, (unsigned)a.npanel), dim3(256), 0, st, a.n, rv, (const double*)a.part_uc,
                       cg_panel_op_blocks(a.n, a.spr_op), (const T*)a.u, (const T*)a.c, a.xx, a.r, a.part_rr, (const CgPanelState*)sn);
}

template <typename T> void cg_panel_finish(hipStream_t st, const CgPanelArgs<T>& a, int cur) {
    if (a.n <= 0 || a.npanel <= 0) return;
    hipLaunchKernelGGL(k_cgp_finish, dim3((unsigned)a.npanel), dim3(256), 0, st, (const double*)a.part_rr, cg_panel_vec_blocks(a.n), a.state + (int64_t)cur * 16 * a.npanel,
                       a.max_it);
}

template <typename T> void cg_panel_post(hipStream_t st, const CgPanelArgs<T>& a) {
    if (a.n <= 0 || a.m <= 0 || a.npanel <= 0) return;
    with_spr(a.A.spr, [&](auto S) {
        constexpr int SPR = decltype(S)::value;
        const dim3 grid((unsigned)cgp_groups(a.m, rpb_of<SPR>()), (unsigned)a.npanel);
        if (a.rho_col) hipLaunchKernelGGL((k_cgp_post_rows<T, SPR, true>), grid, dim3(PS_THREADS), 0, st, a.m, a.n, a.A.rp, a.A.ci, a.A.va, (const T*)a.xx, a.z, a.zp, a.y,
                                          a.lo, a.hi, a.active, a.alpha, a.rho, a.rho_row, a.rho1_row, a.rho_col, a.rho1_col);
        else hipLaunchKernelGGL((k_cgp_post_rows<T, SPR, false>), grid, dim3(PS_THREADS), 0, st, a.m, a.n, a.A.rp, a.A.ci, a.A.va, (const T*)a.xx, a.z, a.zp, a.y,
                                a.lo, a.hi, a.active, a.alpha, a.rho, a.rho_row, a.rho1_row, a.rho_col, a.rho1_col);
    });
    const int64_t per = (int64_t)a.n * 16, total = per * a.npanel;
    hipLaunchKernelGGL((k_cgp_post_x<T>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, per, total, (const T*)a.xx, a.x, a.xp, a.active, a.alpha);
}

template <typename T> void cg_panel_w(hipStream_t st, const CgPanelArgs<T>& a, T* w) {
    if (a.m <= 0 || a.npanel <= 0) return;
    const int64_t per = (int64_t)a.m * 16, total = per * a.npanel;
    hipLaunchKernelGGL((k_cgp_w<T>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, per, total, (const T*)a.z, (const T*)a.y, a.active, a.rho_row, a.rho_col, w);
}

#define INST(T)                                                                                  \
    template void cg_panel_w<T>(hipStream_t, const CgPanelArgs<T>&, T*);                         \
    template void cg_panel_begin<T>(hipStream_t, const CgPanelArgs<T>&);                         \
    template void cg_panel_iteration<T>(hipStream_t, const CgPanelArgs<T>&, int, bool);          \
    template void cg_panel_finish<T>(hipStream_t, const CgPanelArgs<T>&, int);                   \
    template void cg_panel_post<T>(hipStream_t, const CgPanelArgs<T>&);
INST(double)
INST(float)
#undef INST

}  // namespace qps
