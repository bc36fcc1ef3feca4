// k_shared_polish.hip -- the polishing step (SolveQuadraticProgram.m:289-325) for every column of a shared-matrix batch at once: the panel form of the
// kernels of qps_polish.hip.
//
// A KKT vector of the batch is the pair of panel arrays [npanel][rowsN][16] (the x block) followed by [npanel][rowsM][16] (the multiplier block, full length m
// with a 0/1 mask as in qps_polish.hip); row r of a column is row r of the first array for r < rowsN and row r - rowsN of the second otherwise, so the two
// halves are what the handle's panel products read and write.  The products with K are not here: the host driver (SharedFamilySolver::polish_panels) calls the
// handle's check_products for A v_x, P v_x and A'(mask v_lambda), and the first kernel that reads K v or KK v forms it from those three panels (kk_entry).
//
// MINRES (Paige & Saunders 1975) runs one SharedPolishState per column, all columns in lockstep, scalars in double and vectors in T, with the recurrences and
// the ping-ponged state of the single-vector kernels.  A column whose state is `done` is skipped by every vector kernel and stays frozen, like a column the
// active mask of the ADMM loop has stopped.
//
// Reductions: a thread owns (row, col = tid & 15) and adds its rows in row order; the lanes of equal column meet through two shuffles (xor 16, xor 32), the four
// waves through LDS in wave order, and one partial per (column, workgroup) goes to memory.  Every consumer adds a column's partials in workgroup order.  The
// number of workgroups depends on rowsN + rowsM only (shared_polish_blocks), so a column's sums -- hence its iterates -- do not depend on `count`, on the panel
// it sits in or on the other columns.  No float atomics, no scratch.
#include <algorithm>

#include "qps_kernels.h"

namespace qps {

namespace {

using G = SharedPolishGeom;
using State = SharedPolishState;

__device__ __forceinline__ int64_t vec_index(const G& g, int P, int r, int col) {
    return r < g.rowsN ? ((int64_t)P * g.rowsN + r) * 16 + col : (int64_t)g.npanel * g.rowsN * 16 + ((int64_t)P * g.rowsM + (r - g.rowsN)) * 16 + col;
}
// entry r of  K v + delta blkdiag(I, -I) v  from the panels of the products: (P v_x + delta v_x) + A'wl,  mask (A v_x) - delta wl  with wl = mask v_lambda  (:304-305)
template <typename T>
__device__ __forceinline__ T kk_entry(const G& g, int P, int r, int col, T delta, T vi, const T* __restrict__ wl, const T* __restrict__ mask,
                                      const T* __restrict__ Ax, const T* __restrict__ Px, const T* __restrict__ Aty) {
    if (r < g.rowsN) { const int64_t j = ((int64_t)P * g.rowsN + r) * 16 + col; return (Px[j] + delta * vi) + Aty[j]; }
    const int64_t j = ((int64_t)P * g.rowsM + (r - g.rowsN)) * 16 + col;
    return mask[j] * Ax[j] - delta * wl[j];
}
// the sum of d over the rows of this workgroup, per column: valid in threads 0..15 (col = tid)
__device__ __forceinline__ double block_col_sum(double d, double (*red)[16]) {
    d += __shfl_xor(d, 16); d += __shfl_xor(d, 32);            // a + b is the same double on both lanes of a pair
    if ((threadIdx.x & 63) < 16) red[threadIdx.x >> 6][threadIdx.x & 15] = d;
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x < 16) r = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
    __syncthreads();
    return r;
}
// a column's partials added in workgroup order, returned to every thread of that column
__device__ __forceinline__ double col_total(const double* __restrict__ part, int nblk, int P, double* sh) {
    if (threadIdx.x < 16) {
        const double* p = part + (int64_t)(P * 16 + threadIdx.x) * nblk;
        double d = 0.0;
        for (int j = 0; j < nblk; ++j) d += p[j];
        sh[threadIdx.x] = d;
    }
    __syncthreads();
    const double r = sh[threadIdx.x & 15];
    __syncthreads();
    return r;
}

// mask = (y < 0 || y > 0), g = [-q ; y < 0 ? l : (y > 0 ? u : 0)], counts[2 b], counts[2 b + 1] = numL, numU of column b      SolveQuadraticProgram.m:293-299
template <typename T>
__global__ __launch_bounds__(256) void k_sp_setup(G g, const T* __restrict__ q, const T* __restrict__ l, const T* __restrict__ u, const T* __restrict__ y,
                                                  T* __restrict__ mask, T* __restrict__ gv, int* __restrict__ counts) {
    const int P = blockIdx.y, col = threadIdx.x & 15, rl = threadIdx.x >> 4;
    int nl = 0, nu = 0;
    for (int r = blockIdx.x * 16 + rl; r < g.rowsN + g.rowsM; r += gridDim.x * 16) {
        const int64_t i = vec_index(g, P, r, col);
        if (r < g.rowsN) { gv[i] = r < g.n ? -q[((int64_t)P * g.rowsN + r) * 16 + col] : T(0); continue; }
        const int rm = r - g.rowsN;
        const int64_t j = ((int64_t)P * g.rowsM + rm) * 16 + col;
        T mk = T(0), b = T(0);
        if (rm < g.m) {
            const T yi = y[j];
            if (yi < T(0)) { mk = T(1); b = l[j]; ++nl; }
            else if (yi > T(0)) { mk = T(1); b = u[j]; ++nu; }
        }
        mask[j] = mk; gv[i] = b;
    }
    nl += __shfl_xor(nl, 16); nl += __shfl_xor(nl, 32);
    nu += __shfl_xor(nu, 16); nu += __shfl_xor(nu, 32);
    if ((threadIdx.x & 63) < 16) {                              // integer sums: any order gives the same count
        if (nl) atomicAdd(&counts[2 * (P * 16 + col)], nl);
        if (nu) atomicAdd(&counts[2 * (P * 16 + col) + 1], nu);
    }
}
// the set-up of qps_adjoint_shared, the twin of k_sp_setup: mask = (y < 0 || y > 0), g = [g_x ; 0], counts as there
template <typename T>
__global__ __launch_bounds__(256) void k_sp_adjoint_setup(G g, const T* __restrict__ gx, const T* __restrict__ y, T* __restrict__ mask, T* __restrict__ gv,
                                                          int* __restrict__ counts) {
    const int P = blockIdx.y, col = threadIdx.x & 15, rl = threadIdx.x >> 4;
    int nl = 0, nu = 0;
    for (int r = blockIdx.x * 16 + rl; r < g.rowsN + g.rowsM; r += gridDim.x * 16) {
        const int64_t i = vec_index(g, P, r, col);
        if (r < g.rowsN) { gv[i] = r < g.n ? gx[((int64_t)P * g.rowsN + r) * 16 + col] : T(0); continue; }
        const int rm = r - g.rowsN;
        const int64_t j = ((int64_t)P * g.rowsM + rm) * 16 + col;
        T mk = T(0);
        if (rm < g.m) {
            const T yi = y[j];
            if (yi < T(0)) { mk = T(1); ++nl; }
            else if (yi > T(0)) { mk = T(1); ++nu; }
        }
        mask[j] = mk; gv[i] = T(0);
    }
    nl += __shfl_xor(nl, 16); nl += __shfl_xor(nl, 32);
    nu += __shfl_xor(nu, 16); nu += __shfl_xor(nu, 32);
    if ((threadIdx.x & 63) < 16) {                              // integer sums: any order gives the same count
        if (nl) atomicAdd(&counts[2 * (P * 16 + col)], nl);
        if (nu) atomicAdd(&counts[2 * (P * 16 + col) + 1], nu);
    }
}
// the read-out of qps_adjoint_shared: dq = -t_x, dl = t_lambda where y < 0, du = t_lambda where y > 0; a column that is not live gives zeros and its t is
// cleared, so that what sums over the columns afterwards leaves it out
template <typename T>
__global__ __launch_bounds__(256) void k_sp_adjoint_readout(G g, const int* __restrict__ live, const T* __restrict__ y, T* __restrict__ t, T* __restrict__ dq,
                                                            T* __restrict__ dl, T* __restrict__ du) {
    const int P = blockIdx.y, col = threadIdx.x & 15, rl = threadIdx.x >> 4;
    const bool on = live[P * 16 + col] != 0;
    for (int r = blockIdx.x * 16 + rl; r < g.rowsN + g.rowsM; r += gridDim.x * 16) {
        const int64_t i = vec_index(g, P, r, col);
        if (!on) t[i] = T(0);
        const T v = on ? t[i] : T(0);
        if (r < g.rowsN) { dq[((int64_t)P * g.rowsN + r) * 16 + col] = on ? -v : T(0); continue; }
        const int rm = r - g.rowsN;
        const int64_t j = ((int64_t)P * g.rowsM + rm) * 16 + col;
        const T yi = rm < g.m ? y[j] : T(0);
        dl[j] = yi < T(0) ? v : T(0);
        du[j] = yi > T(0) ? v : T(0);
    }
}
// wl = mask v_lambda (every column)
template <typename T> __global__ __launch_bounds__(256) void k_sp_wl(G g, const T* __restrict__ mask, const T* __restrict__ v, T* __restrict__ wl) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, len = (int64_t)g.npanel * g.rowsM * 16;
    if (i < len) wl[i] = mask[i] * v[(int64_t)g.npanel * g.rowsN * 16 + i];
}
// rhs = g - K t for the live columns (the products are those of t and wl = mask t_lambda)                                        :315
template <typename T>
__global__ __launch_bounds__(256) void k_sp_rhs(G g, const int* __restrict__ live, const T* __restrict__ gv, const T* __restrict__ t, const T* __restrict__ wl,
                                                const T* __restrict__ mask, const T* __restrict__ Ax, const T* __restrict__ Px, const T* __restrict__ Aty,
                                                T* __restrict__ rhs) {
    const int P = blockIdx.y, col = threadIdx.x & 15, rl = threadIdx.x >> 4;
    if (!live[P * 16 + col]) return;
    for (int r = blockIdx.x * 16 + rl; r < g.rowsN + g.rowsM; r += gridDim.x * 16) {
        const int64_t i = vec_index(g, P, r, col);
        rhs[i] = gv[i] - kk_entry<T>(g, P, r, col, T(0), t[i], wl, mask, Ax, Px, Aty);
    }
}
// r1 = b - KK x0, r2 = r1, w = w2 = 0; partials of ||r1||^2 and ||b||^2 per (column, workgroup)
template <typename T>
__global__ __launch_bounds__(256) void k_sp_begin(G g, const int* __restrict__ live, T delta, const T* __restrict__ b, const T* __restrict__ x0,
                                                  const T* __restrict__ wl, const T* __restrict__ mask, const T* __restrict__ Ax, const T* __restrict__ Px,
                                                  const T* __restrict__ Aty, T* __restrict__ r1, T* __restrict__ r2, T* __restrict__ w0, T* __restrict__ w1,
                                                  double* __restrict__ pa, double* __restrict__ pb) {
    __shared__ double red[4][16];
    const int P = blockIdx.y, col = threadIdx.x & 15, rl = threadIdx.x >> 4;
    const bool on = live[P * 16 + col] != 0;
    double d = 0.0, e = 0.0;
    for (int r = blockIdx.x * 16 + rl; on && r < g.rowsN + g.rowsM; r += gridDim.x * 16) {
        const int64_t i = vec_index(g, P, r, col);
        const T bi = b[i], ri = bi - kk_entry<T>(g, P, r, col, delta, x0[i], wl, mask, Ax, Px, Aty);
        r1[i] = ri; r2[i] = ri; w0[i] = T(0); w1[i] = T(0);
        d += (double)ri * (double)ri; e += (double)bi * (double)bi;
    }
    d = block_col_sum(d, red); e = block_col_sum(e, red);
    if (threadIdx.x < 16) { const int64_t o = (int64_t)(P * 16 + col) * gridDim.x + blockIdx.x; pa[o] = d; pb[o] = e; }
}
// one thread per column: the state MINRES starts from; a column that is not live is born done
__global__ void k_sp_begin_final(int cols, int nblk, const int* __restrict__ live, const double* __restrict__ pa, const double* __restrict__ pb,
                                 State* __restrict__ st, double tol, int maxit) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= cols) return;
    State s;
    s.beta = 0.0; s.oldb = 0.0; s.dbar = 0.0; s.epsln = 0.0; s.phibar = 0.0; s.cs = -1.0; s.sn = 0.0; s.bnorm = 0.0; s.tol = tol; s.alfa = 0.0;
    s.itn = 0; s.maxit = maxit; s.done = 1; s.flag = 1;
    if (live[b]) {
        double d = 0.0, e = 0.0;
        for (int j = 0; j < nblk; ++j) { d += pa[(int64_t)b * nblk + j]; e += pb[(int64_t)b * nblk + j]; }
        const double beta1 = sqrt(d), bnorm = sqrt(e);
        s.beta = beta1; s.phibar = beta1; s.bnorm = bnorm; s.done = 0;
        if (bnorm == 0.0) { s.done = 1; s.flag = 0; s.phibar = 0.0; }                        // b == 0: x = 0, converged (k_sp_add clears x)
        else if (!(beta1 == beta1) || isinf(beta1) || !(bnorm == bnorm) || isinf(bnorm)) { s.done = 1; s.flag = 1; }
        else if (beta1 <= tol * bnorm) { s.done = 1; s.flag = 0; }
        else if (maxit <= 0) { s.done = 1; s.flag = 1; }
    }
    st[b] = s; st[cols + b] = s;
}
// c = KK y from the products of y (= r2) and wl = mask y_lambda; partial of  alfa = v'(A v - (beta/oldb) r1),  v = y / beta,  A v = c / beta
template <typename T>
__global__ __launch_bounds__(256) void k_sp_alfa(G g, const State* __restrict__ st, T delta, const T* __restrict__ y, const T* __restrict__ wl,
                                                 const T* __restrict__ mask, const T* __restrict__ Ax, const T* __restrict__ Px, const T* __restrict__ Aty,
                                                 const T* __restrict__ r1, T* __restrict__ c, double* __restrict__ pa) {
    __shared__ double red[4][16];
    const int P = blockIdx.y, col = threadIdx.x & 15, rl = threadIdx.x >> 4;
    const State* sc = st + P * 16 + col;
    const bool on = !sc->done;
    T s = T(0), f = T(0);
    if (on) { s = (T)(1.0 / sc->beta); f = sc->itn >= 1 ? (T)(sc->beta / sc->oldb) : T(0); }
    double d = 0.0;
    for (int r = blockIdx.x * 16 + rl; on && r < g.rowsN + g.rowsM; r += gridDim.x * 16) {
        const int64_t i = vec_index(g, P, r, col);
        const T yi = y[i], ci = kk_entry<T>(g, P, r, col, delta, yi, wl, mask, Ax, Px, Aty);
        c[i] = ci;
        const T t = s * ci - f * r1[i];
        d += (double)(s * yi) * (double)t;
    }
    d = block_col_sum(d, red);
    if (threadIdx.x < 16 && on) pa[(int64_t)(P * 16 + col) * gridDim.x + blockIdx.x] = d;
}
// y_new = A v - (beta/oldb) r1 - (alfa/beta) r2, written over r1, and wl = mask y_new_lambda for the next product; partial ||y_new||^2
template <typename T>
__global__ __launch_bounds__(256) void k_sp_lanczos(G g, State* __restrict__ st, const double* __restrict__ pa, const T* __restrict__ c, T* __restrict__ r1,
                                                    const T* __restrict__ r2, const T* __restrict__ mask, T* __restrict__ wl, double* __restrict__ pb) {
    __shared__ double red[4][16];
    __shared__ double sh[16];
    const int P = blockIdx.y, col = threadIdx.x & 15, rl = threadIdx.x >> 4;
    State* sc = st + P * 16 + col;
    const bool on = !sc->done;
    const double alfa = col_total(pa, gridDim.x, P, sh);
    T s = T(0), f = T(0), h = T(0);
    if (on) { s = (T)(1.0 / sc->beta); f = sc->itn >= 1 ? (T)(sc->beta / sc->oldb) : T(0); h = (T)(alfa / sc->beta); }
    double d = 0.0;
    for (int r = blockIdx.x * 16 + rl; on && r < g.rowsN + g.rowsM; r += gridDim.x * 16) {
        const int64_t i = vec_index(g, P, r, col);
        T t = s * c[i] - f * r1[i];
        t -= h * r2[i];
        r1[i] = t;
        if (r >= g.rowsN) { const int64_t j = ((int64_t)P * g.rowsM + (r - g.rowsN)) * 16 + col; wl[j] = mask[j] * t; }
        d += (double)t * (double)t;
    }
    d = block_col_sum(d, red);
    if (threadIdx.x < 16 && on) { pb[(int64_t)(P * 16 + col) * gridDim.x + blockIdx.x] = d; if (blockIdx.x == 0) sc->alfa = alfa; }
}
// Givens rotation, w = (v - oldeps w1 - delta w2) / gamma (over w1's buffer), x += phi w; workgroup 0 of a panel publishes the next states of its columns
template <typename T>
__global__ __launch_bounds__(256) void k_sp_update(G g, const State* __restrict__ cur, State* __restrict__ nxt, const double* __restrict__ pb,
                                                   const T* __restrict__ vsrc, T* __restrict__ w1, const T* __restrict__ w2, T* __restrict__ x) {
    __shared__ double sh[16];
    const int P = blockIdx.y, col = threadIdx.x & 15, rl = threadIdx.x >> 4;
    const State c0 = cur[P * 16 + col];
    const bool on = !c0.done;
    const double beta_new = sqrt(col_total(pb, gridDim.x, P, sh));
    const double beta = c0.beta, alfa = c0.alfa, cs0 = c0.cs, sn0 = c0.sn, dbar0 = c0.dbar;
    const double oldeps = c0.epsln;
    const double delta = cs0 * dbar0 + sn0 * alfa;
    const double gbar = sn0 * dbar0 - cs0 * alfa;
    const double epsln = sn0 * beta_new;
    const double dbar = -cs0 * beta_new;
    const double gamma = fmax(sqrt(gbar * gbar + beta_new * beta_new), 2.220446049250313e-16);
    const double cs = gbar / gamma, sn = beta_new / gamma;
    const double phi = cs * c0.phibar, phibar = sn * c0.phibar;
    for (int r = blockIdx.x * 16 + rl; on && r < g.rowsN + g.rowsM; r += gridDim.x * 16) {
        const int64_t i = vec_index(g, P, r, col);
        const T v = (T)(1.0 / beta) * vsrc[i];
        const T wn = (v - (T)oldeps * w1[i] - (T)delta * w2[i]) / (T)gamma;
        w1[i] = wn;
        x[i] += (T)phi * wn;
    }
    if (blockIdx.x == 0 && threadIdx.x < 16) {
        State s = c0;
        if (on) {
            s.oldb = beta; s.beta = beta_new; s.dbar = dbar; s.epsln = epsln; s.phibar = phibar; s.cs = cs; s.sn = sn; s.itn = c0.itn + 1;
            if (!(phibar == phibar) || isinf(phibar)) { s.done = 1; s.flag = 1; }
            else if (phibar <= s.tol * s.bnorm) { s.done = 1; s.flag = 0; }
            else if (beta_new == 0.0) { s.done = 1; s.flag = 0; }
            else if (s.itn >= s.maxit) { s.done = 1; s.flag = 1; }
        }
        nxt[P * 16 + col] = s;
    }
}
// t += tt for the live columns (:319); a column whose right-hand side was zero takes tt = 0 first
template <typename T>
__global__ __launch_bounds__(256) void k_sp_add(G g, const int* __restrict__ live, const State* __restrict__ st, T* __restrict__ t, T* __restrict__ tt) {
    const int P = blockIdx.y, col = threadIdx.x & 15, rl = threadIdx.x >> 4;
    if (!live[P * 16 + col]) return;
    const bool zero = st[P * 16 + col].bnorm == 0.0;
    for (int r = blockIdx.x * 16 + rl; r < g.rowsN + g.rowsM; r += gridDim.x * 16) {
        const int64_t i = vec_index(g, P, r, col);
        if (zero) tt[i] = T(0);
        else t[i] += tt[i];
    }
}
// x = t_x for the columns whose last MINRES call converged (:322-325); the others keep their x
template <typename T>
__global__ __launch_bounds__(256) void k_sp_select(G g, const int* __restrict__ take, const T* __restrict__ t, T* __restrict__ x) {
    const int P = blockIdx.y, col = threadIdx.x & 15, rl = threadIdx.x >> 4;
    if (!take[P * 16 + col]) return;
    for (int r = blockIdx.x * 16 + rl; r < g.rowsN; r += gridDim.x * 16) {
        const int64_t i = ((int64_t)P * g.rowsN + r) * 16 + col;
        x[i] = t[i];
    }
}

inline dim3 grid_of(const G& g) { return dim3((unsigned)shared_polish_blocks(g.rowsN, g.rowsM), (unsigned)g.npanel); }

}  // namespace

// workgroups per panel of every row kernel: a function of the vector length alone (two rows per thread up to 64 workgroups, a longer stride beyond)
int shared_polish_blocks(int rowsN, int rowsM) { return std::max(1, std::min(64, (rowsN + rowsM + 31) / 32)); }

template <typename T>
void shared_polish_setup(hipStream_t st, const SharedPolishGeom& g, const T* q, const T* l, const T* u, const T* y, T* mask, T* gv, int* counts) {
    hipLaunchKernelGGL((k_sp_setup<T>), grid_of(g), dim3(256), 0, st, g, q, l, u, y, mask, gv, counts);
}
template <typename T> void shared_adjoint_setup(hipStream_t st, const SharedPolishGeom& g, const T* gx, const T* y, T* mask, T* gv, int* counts) {
    hipLaunchKernelGGL((k_sp_adjoint_setup<T>), grid_of(g), dim3(256), 0, st, g, gx, y, mask, gv, counts);
}
template <typename T> void shared_adjoint_readout(hipStream_t st, const SharedPolishGeom& g, const int* live, const T* y, T* t, T* dq, T* dl, T* du) {
    hipLaunchKernelGGL((k_sp_adjoint_readout<T>), grid_of(g), dim3(256), 0, st, g, live, y, t, dq, dl, du);
}
template <typename T> void shared_polish_wl(hipStream_t st, const SharedPolishGeom& g, const T* mask, const T* v, T* wl) {
    const int64_t len = (int64_t)g.npanel * g.rowsM * 16;
    hipLaunchKernelGGL((k_sp_wl<T>), dim3((unsigned)((len + 255) / 256)), dim3(256), 0, st, g, mask, v, wl);
}
template <typename T>
void shared_polish_rhs(hipStream_t st, const SharedPolishGeom& g, const int* live, const T* gv, const T* t, const SharedPolishProducts<T>& k, T* rhs) {
    hipLaunchKernelGGL((k_sp_rhs<T>), grid_of(g), dim3(256), 0, st, g, live, gv, t, k.wl, k.mask, k.Ax, k.Px, k.Aty, rhs);
}
template <typename T>
void shared_polish_begin(hipStream_t st, const SharedPolishGeom& g, const int* live, T delta, const T* b, const T* x0, const SharedPolishProducts<T>& k, T* r1,
                         T* r2, T* w0, T* w1, double* pa, double* pb, SharedPolishState* state, double tol, int maxit) {
    const int cols = g.npanel * 16;
    hipLaunchKernelGGL((k_sp_begin<T>), grid_of(g), dim3(256), 0, st, g, live, delta, b, x0, k.wl, k.mask, k.Ax, k.Px, k.Aty, r1, r2, w0, w1, pa, pb);
    hipLaunchKernelGGL(k_sp_begin_final, dim3((unsigned)((cols + 63) / 64)), dim3(64), 0, st, cols, shared_polish_blocks(g.rowsN, g.rowsM), live, pa, pb, state, tol,
                       maxit);
}
template <typename T>
void shared_polish_step(hipStream_t st, const SharedPolishGeom& g, SharedPolishState* cur, SharedPolishState* nxt, T delta, const SharedPolishProducts<T>& k,
                        T* c, T* r1, T* r2, T* w1, const T* w2, T* x, double* pa, double* pb) {
    hipLaunchKernelGGL((k_sp_alfa<T>), grid_of(g), dim3(256), 0, st, g, cur, delta, r2, k.wl, k.mask, k.Ax, k.Px, k.Aty, r1, c, pa);
    hipLaunchKernelGGL((k_sp_lanczos<T>), grid_of(g), dim3(256), 0, st, g, cur, pa, c, r1, r2, k.mask, k.wl, pb);
    hipLaunchKernelGGL((k_sp_update<T>), grid_of(g), dim3(256), 0, st, g, cur, nxt, pb, r2, w1, w2, x);
}
template <typename T> void shared_polish_add(hipStream_t st, const SharedPolishGeom& g, const int* live, const SharedPolishState* state, T* t, T* tt) {
    hipLaunchKernelGGL((k_sp_add<T>), grid_of(g), dim3(256), 0, st, g, live, state, t, tt);
}
template <typename T> void shared_polish_select(hipStream_t st, const SharedPolishGeom& g, const int* take, const T* t, T* x) {
    hipLaunchKernelGGL((k_sp_select<T>), grid_of(g), dim3(256), 0, st, g, take, t, x);
}

#define INST(T)                                                                                                                                              \
    template void shared_polish_setup<T>(hipStream_t, const SharedPolishGeom&, const T*, const T*, const T*, const T*, T*, T*, int*);                        \
    template void shared_adjoint_setup<T>(hipStream_t, const SharedPolishGeom&, const T*, const T*, T*, T*, int*);                                         \
    template void shared_adjoint_readout<T>(hipStream_t, const SharedPolishGeom&, const int*, const T*, T*, T*, T*, T*);                                    \
    template void shared_polish_wl<T>(hipStream_t, const SharedPolishGeom&, const T*, const T*, T*);                                                         \
    template void shared_polish_rhs<T>(hipStream_t, const SharedPolishGeom&, const int*, const T*, const T*, const SharedPolishProducts<T>&, T*);            \
    template void shared_polish_begin<T>(hipStream_t, const SharedPolishGeom&, const int*, T, const T*, const T*, const SharedPolishProducts<T>&, T*, T*, T*, \
                                         T*, double*, double*, SharedPolishState*, double, int);                                                             \
    template void shared_polish_step<T>(hipStream_t, const SharedPolishGeom&, SharedPolishState*, SharedPolishState*, T, const SharedPolishProducts<T>&, T*, \
                                        T*, T*, T*, const T*, T*, double*, double*);                                                                         \
    template void shared_polish_add<T>(hipStream_t, const SharedPolishGeom&, const int*, const SharedPolishState*, T*, T*);                                  \
    template void shared_polish_select<T>(hipStream_t, const SharedPolishGeom&, const int*, const T*, T*);
INST(double)
INST(float)
#undef INST

}  // namespace qps
