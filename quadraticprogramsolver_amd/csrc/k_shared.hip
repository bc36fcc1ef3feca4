// k_shared.hip -- loop kernels of the shared-matrix batch (qps_create_dense_shared_batch): many QPs on ONE P and ONE A.
//
// With the matrices shared, every product of an ADMM iteration is "row-major matrix x 16-column panel": the matrix operand is streamed
// once and serves all columns, the right-hand operand is a panel of 16 QPs.  That is the shape of v_mfma_f64_16x16x4_f64 /
// v_mfma_f32_16x16x4_f32 (D[16 rows][16 QPs] += M[16 rows][4 k] * X[4 k][16 QPs]).
//
// State layout: a length-R vector of `count` QPs is a stack of panels [panel][row][16] (QP b = panel b / 16, column b % 16), rows padded like
// the single-QP vectors (NP / MP), `count` padded to a multiple of 16 with columns that stay inactive and zero.
//
// One kernel, k_panel<T, TRI, EPI, PB, waves, staged>, does every product:
//   * a workgroup of 8 (or 16) waves owns 16 matrix rows and PB panels; the k range of those rows is cut into steps of 32 columns dealt
//     round-robin to the waves (wave w takes steps w, w + waves, ...), so a workgroup streams its rows front to back;
//   * per step a lane loads 16 bytes per load instruction, non-temporal for the constraint matrix: whole 32-column rows of the tile (full
//     cache lines), turned into the MFMA operand layout (row = lane & 15, k group = lane >> 4) through the wave's own LDS tile; matrices
//     small enough to stay cached skip LDS and load in operand layout with 16 waves per workgroup.  The matching panel rows go straight
//     into registers; the accumulators (PB tiles) stay in VGPRs; the next step's loads are issued before the current step's MFMAs (two
//     register sets);
//   * the partial tiles of the waves meet in LDS and are added in wave order -- every output element is its own dot product with a summation
//     order that depends on the matrix shape only, never on `count` or on the QP's position: column b of a batch is bit-identical to the same
//     data solved alone;
//   * the row-wise part of the iteration runs as the epilogue on the summed tile (EPI), per column, honouring the active mask.
// TRI: 0 full rows, 1 columns <= row (forward sweep over the sweep matrix S), 2 columns >= row (backward sweep).
// No float atomics, no scratch; the check norms use the u64 atomicMax scheme of k_loop.hip with 16 slots per column.
#include <hip/hip_ext.h>

#include <algorithm>

#include "qps_kernels.h"
#include "wave_reduce.h"

namespace qps {

namespace {

typedef double sd4 __attribute__((ext_vector_type(4)));
typedef float sf4 __attribute__((ext_vector_type(4)));

template <typename T> struct PanelMfma;
template <> struct PanelMfma<double> {
    using acc_t = sd4;
    static __device__ __forceinline__ acc_t run(double a, double b, acc_t c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
    // C/D layout of v_mfma_f64_16x16x4_f64: col = lane & 15, row = (lane >> 4) + 4 * reg
    static __device__ __forceinline__ int row(int lane, int reg) { return (lane >> 4) + 4 * reg; }
};
template <> struct PanelMfma<float> {
    using acc_t = sf4;
    static __device__ __forceinline__ acc_t run(float a, float b, acc_t c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
    // C/D layout of v_mfma_f32_16x16x4_f32: col = lane & 15, row = (lane >> 4) * 4 + reg
    static __device__ __forceinline__ int row(int lane, int reg) { return (lane >> 4) * 4 + reg; }
};

__device__ __forceinline__ unsigned long long sh_absbits(double v) { return (unsigned long long)__double_as_longlong(fabs(v)); }
__device__ __forceinline__ unsigned long long sh_umax(unsigned long long a, unsigned long long b) { return a > b ? a : b; }

// w = rho_i z - y, the operand of the next right-hand side (LinearSystemSolvers.jl:134-135): ONE expression for the row epilogues of k_panel and for k_panel_w,
// so that a w re-formed from a stored (z, y) carries the bits the row update would have left behind
template <typename T> __device__ __forceinline__ T panel_w_of(T rr, T z, T y) { return rr * z - y; }

// waves per workgroup (k split): 8, or 16 for matrices small enough to sit in the caches (shared_panel_small)
constexpr int SH_KS = 32;     // matrix columns per step

template <typename T, int TRI, int PB, bool STG>
struct PanelStep {
    static constexpr int VN = VecOf<T>::N;          // elements per 16-byte load
    static constexpr int U = SH_KS / (4 * VN);      // 16-byte loads per matrix row and step
    typedef T NV __attribute__((ext_vector_type(VN)));
    using acc_t = typename PanelMfma<T>::acc_t;

    static constexpr int LPR = SH_KS / VN;          // staged form: lanes per matrix row of a step (16 fp64, 8 fp32) ...
    static constexpr int RPI = 64 / LPR;            // ... and rows per load instruction (RPI * U = 16)
    static constexpr int LROW = SH_KS + 16 / (int)sizeof(T);   // LDS row stride of a staged tile (elements): 32 columns + 16 bytes

    // Direct form (STG = false).  lane (lc = lane & 15, g = lane >> 4): matrix row r0 + lc, columns kc + 4 VN u + VN g + j -- the MFMA
    // operand layout: one load instruction touches 16 rows x 64 B.
    // Staged form (STG = true): load u of the wave covers rows RPI u + lane / LPR whole (SH_KS columns, full 128-byte lines: measured
    // 4.7-5.0 TB/s against 3.8-3.9 TB/s for the 64-byte pieces on the n = 4096, m = 8192 passes); stage() turns the tile into the operand
    // layout through the wave's own LDS tile.  arow points at the lane's first element either way.
    // Both forms: panel rows of the same k, column lc.
    static __device__ __forceinline__ void load(NV (&A)[U], T (&B)[PB][U][VN], const T* arow, const T* const (&bcol)[PB], int kc, int g, int64_t ld) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const NV* src = reinterpret_cast<const NV*>(STG ? arow + kc + (int64_t)(RPI * u) * ld : arow + kc + u * 4 * VN);
            A[u] = (TRI == 0) ? __builtin_nontemporal_load(src) : *src;
        }
#pragma unroll
        for (int pb = 0; pb < PB; ++pb)
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int j = 0; j < VN; ++j) B[pb][u][j] = bcol[pb][(int64_t)(kc + u * 4 * VN + VN * g + j) * 16];
    }
    // staged tile -> operand layout through the wave's own LDS tile `t` (16 rows of LROW elements).  Only this wave touches `t` and a wave's
    // LDS accesses execute in order, so no workgroup barrier is needed; the wave barriers keep the COMPILER from moving the reads (other lanes'
    // data: no per-thread alias) above the writes, or the next step's writes above these reads.
    static __device__ __forceinline__ void stage(NV (&A)[U], T* t, int lane) {
        const int lc = lane & 15, g = lane >> 4;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int u = 0; u < U; ++u) *reinterpret_cast<NV*>(t + (RPI * u + lane / LPR) * LROW + VN * (lane % LPR)) = A[u];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int u = 0; u < U; ++u) A[u] = *reinterpret_cast<const NV*>(t + lc * LROW + 4 * VN * u + VN * g);
    }
    static __device__ __forceinline__ void mac(acc_t (&acc)[PB], NV (&A)[U], const T (&B)[PB][U][VN], int kc, int r0, int lc, int g) {
        if (TRI != 0) {
            // steps that touch the diagonal tile: the other triangle of S holds the mirrored factor, not zeros
            const bool diag = (TRI == 1) ? (kc + SH_KS > r0) : (kc < r0 + 16);
            if (diag) {
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int j = 0; j < VN; ++j) {
                        const int c = kc + u * 4 * VN + VN * g + j, r = r0 + lc;
                        const bool keep = (TRI == 1) ? (c <= r) : (c >= r);
                        A[u][j] = keep ? A[u][j] : T(0);
                    }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int j = 0; j < VN; ++j)
#pragma unroll
                for (int pb = 0; pb < PB; ++pb) acc[pb] = PanelMfma<T>::run(A[u][j], B[pb][u][j], acc[pb]);
    }
};

// EPI: 0 out = s;  1 out = sigma x - q + s (right-hand side, LinearSystemSolvers.jl:136);  2 s = x~: out = s, xp = x, x = alpha s + (1 - alpha) x
// (SolveQuadraticProgram.jl:56-57);  3 s = z~: zp = z, z = clamp(...), y += rho (...), w = rho z - y (:59-61 and the next :134-135);
// 4 = 3 with rho read as diag(rho_i): rho_i and 1 / rho_i of the output row come from a.rho_row / a.rho1_row (two cached loads per output element)
// 5 s = A x~ of a warm start (qps_set_shared_warm_start, mode 2): z = s without projection, w = rho_i z - y with the stored y; rho_i = a.rho_row[row], or a.rho
// when a.rho_row is NULL
template <typename T, int TRI, int EPI, int PB, int SH_NW, bool STG>
__global__ __launch_bounds__(SH_NW * 64) void k_panel(PanelArgs<T> a) {
    using S = PanelStep<T, TRI, PB, STG>;
    using acc_t = typename S::acc_t;
    typedef typename S::NV NV;
    constexpr int VN = S::VN, U = S::U;
    constexpr int RED = SH_NW * PB * 256, STAGE = STG ? SH_NW * 16 * S::LROW : 0;
    __shared__ __attribute__((aligned(16))) T red[RED > STAGE ? RED : STAGE];   // the waves' staging tiles during the k loop, then the partial tiles
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, lc = lane & 15;
    T* const tile = red + w * 16 * S::LROW;
    // Workgroup id -> (row tile, panel group).  The groups of ONE row tile get ids 8 apart: ids are dealt round-robin over the 8 XCDs, so the
    // workgroups that stream the same 16 rows for different panels run on one XCD at about the same time and share one trip to HBM.
    const int nrt = a.rows / 16, npg = (a.npanel + PB - 1) / PB, full = (nrt & ~7) * npg, id = blockIdx.x;
    int rt, pg;
    if (id < full) { const int rem = id % (8 * npg); pg = rem >> 3; rt = id / (8 * npg) * 8 + (rem & 7); }
    else { const int j = id - full, tail = nrt & 7; pg = j / tail; rt = (nrt & ~7) + j % tail; }
    const int r0 = rt * 16, p0 = pg * PB;
    int kbeg = 0, kend = a.K;
    if (TRI == 1) kend = min(a.K, (r0 + 16 + SH_KS - 1) & ~(SH_KS - 1));
    if (TRI == 2) kbeg = r0 & ~(SH_KS - 1);
    const int nsteps = (kend - kbeg) / SH_KS;
    const T* const arow = STG ? a.Mat + (int64_t)(r0 + lane / S::LPR) * a.ld + VN * (lane % S::LPR) : a.Mat + (int64_t)(r0 + lc) * a.ld + VN * g;
    const T* bcol[PB];
#pragma unroll
    for (int pb = 0; pb < PB; ++pb) bcol[pb] = a.B + (int64_t)min(p0 + pb, a.npanel - 1) * a.K * 16 + lc;   // (a ragged last group repeats its last panel)
    acc_t acc[PB];
#pragma unroll
    for (int pb = 0; pb < PB; ++pb)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[pb][i] = T(0);
    NV A0[U], A1[U];
    T B0[PB][U][VN], B1[PB][U][VN];
    int s = w;
    if (s < nsteps) S::load(A0, B0, arow, bcol, kbeg + s * SH_KS, g, a.ld);
    while (s < nsteps) {
        int s1 = s + SH_NW;
        if (s1 < nsteps) S::load(A1, B1, arow, bcol, kbeg + s1 * SH_KS, g, a.ld);
        if (STG) S::stage(A0, tile, lane);
        S::mac(acc, A0, B0, kbeg + s * SH_KS, r0, lc, g);
        s = s1;
        if (s >= nsteps) break;
        s1 = s + SH_NW;
        if (s1 < nsteps) S::load(A0, B0, arow, bcol, kbeg + s1 * SH_KS, g, a.ld);
        if (STG) S::stage(A1, tile, lane);
        S::mac(acc, A1, B1, kbeg + s * SH_KS, r0, lc, g);
        s = s1;
    }
    if (STG) __syncthreads();   // every wave is done with its staging tile before the partial tiles overwrite them
#pragma unroll
    for (int pb = 0; pb < PB; ++pb)
#pragma unroll
        for (int i = 0; i < 4; ++i) red[(w * PB + pb) * 256 + PanelMfma<T>::row(lane, i) * 16 + lc] = acc[pb][i];
    __syncthreads();
    const T alpha1 = T(1) - a.alpha, rho1 = T(1) / a.rho;
    for (int e = tid; e < PB * 256; e += SH_NW * 64) {
        T sum = red[e];
#pragma unroll
        for (int ww = 1; ww < SH_NW; ++ww) sum += red[ww * PB * 256 + e];
        const int pb = e >> 8, row = (e >> 4) & 15, col = e & 15;
        const int P = p0 + pb;
        if (P >= a.npanel) continue;
        const int64_t idx = ((int64_t)P * a.rows + r0 + row) * 16 + col;
        if (EPI == 0) a.out[idx] = sum;
        else if (EPI == 1) a.out[idx] = sum + a.sigma * a.x[idx] - a.q[idx];
        else if (EPI == 2) {
            a.out[idx] = sum;
            if (a.active[P * 16 + col]) {
                const T xo = a.x[idx];
                a.xp[idx] = xo;                                          // :56
                a.x[idx] = a.alpha * sum + alpha1 * xo;                  // :57
            }
        } else if (EPI == 3) {
            if (a.active[P * 16 + col]) {
                const T zo = a.z[idx], yo = a.y[idx];
                a.zp[idx] = zo;                                          // :59
                const T t = a.alpha * sum + alpha1 * zo + rho1 * yo;     // :60
                const T lo = a.l[idx], hi = a.u[idx];
                const T zn = t > hi ? hi : (t < lo ? lo : t);
                const T yn = yo + a.rho * (a.alpha * sum + alpha1 * zo - zn);   // :61
                a.z[idx] = zn; a.y[idx] = yn;
                a.w[idx] = panel_w_of(a.rho, zn, yn);                        // LinearSystemSolvers.jl:134-135 of the next iteration
            }
        } else if (EPI == 4) {
            if (a.active[P * 16 + col]) {
                const T rr = a.rho_row[r0 + row], rr1 = a.rho1_row[r0 + row];   // rho_i, 1 / rho_i: r0 + row < a.rows, the vectors' length
                const T zo = a.z[idx], yo = a.y[idx];
                a.zp[idx] = zo;                                          // :59
                const T t = a.alpha * sum + alpha1 * zo + rr1 * yo;      // :60
                const T lo = a.l[idx], hi = a.u[idx];
                const T zn = t > hi ? hi : (t < lo ? lo : t);
                const T yn = yo + rr * (a.alpha * sum + alpha1 * zo - zn);      // :61
                a.z[idx] = zn; a.y[idx] = yn;
                a.w[idx] = panel_w_of(rr, zn, yn);                           // LinearSystemSolvers.jl:134-135 of the next iteration
            }
        } else {
            if (a.active[P * 16 + col]) {
                const T rr = a.rho_row ? a.rho_row[r0 + row] : a.rho;        // r0 + row < a.rows, the vector's length
                a.z[idx] = sum;
                a.w[idx] = panel_w_of(rr, sum, a.y[idx]);                    // LinearSystemSolvers.jl:134-135 of the first iteration
            }
        }
    }
}

// CheckConvergence (SolveQuadraticProgram.jl:79-112), per column: the nine inf-norms of k_check_norms over panels.
// slots (16 per column): 0 ||Ax-z|| 1 ||Px+q+A'y|| 2 ||Ax|| 3 ||z|| 4 ||Px|| 5 ||A'y|| 6 ||q|| 7 ||x-xp|| 8 ||z-zp||
// EQ (qps_set_shared_equilibration): the panels hold the scaled iterates; every term goes back to the caller's units before its norm is taken (OSQP 5.1) --
// E^-1 on the m-rows, D^-1 on P x, q, A'y and their sum, D on x - xp, with D_j = 2^kd[j], E_i = 2^ke[i].  Differences are formed in T as without the
// scaling, then moved by the power of two in double (exact).
template <typename T, bool EQ>
__device__ __forceinline__ void shared_norms_body(int n, int m, int NP, int MP, const T* __restrict__ Ax, const T* __restrict__ Px, const T* __restrict__ Aty,
                                                  const T* __restrict__ q, const T* __restrict__ x, const T* __restrict__ xp, const T* __restrict__ z,
                                                  const T* __restrict__ zp, unsigned long long* __restrict__ slots, const int* __restrict__ kd,
                                                  const int* __restrict__ ke) {
    const int P = blockIdx.y, col = threadIdx.x & 15, rl = threadIdx.x >> 4;
    const int64_t on = (int64_t)P * NP * 16 + col, om = (int64_t)P * MP * 16 + col;
    unsigned long long v[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) v[k] = 0ull;
    for (int r = blockIdx.x * 16 + rl; r < max(n, m); r += gridDim.x * 16) {
        if (r < m) {
            const int64_t i = om + (int64_t)r * 16;
            const int s = EQ ? -ke[r] : 0;
            auto nrm = [&](T t) { return sh_absbits(EQ ? ldexp((double)t, s) : (double)t); };
            v[0] = sh_umax(v[0], nrm(Ax[i] - z[i]));   // differences are formed in T (k_loop.hip)
            v[2] = sh_umax(v[2], nrm(Ax[i]));
            v[3] = sh_umax(v[3], nrm(z[i]));
            v[8] = sh_umax(v[8], nrm(z[i] - zp[i]));
        }
        if (r < n) {
            const int64_t i = on + (int64_t)r * 16;
            const int s = EQ ? -kd[r] : 0;
            auto nrm = [&](T t) { return sh_absbits(EQ ? ldexp((double)t, s) : (double)t); };
            v[1] = sh_umax(v[1], nrm(Px[i] + q[i] + Aty[i]));
            v[4] = sh_umax(v[4], nrm(Px[i]));
            v[5] = sh_umax(v[5], nrm(Aty[i]));
            v[6] = sh_umax(v[6], nrm(q[i]));
            v[7] = sh_umax(v[7], sh_absbits(EQ ? ldexp((double)(x[i] - xp[i]), -s) : (double)(x[i] - xp[i])));
        }
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        v[k] = sh_umax(v[k], __shfl_xor(v[k], 16));
        v[k] = sh_umax(v[k], __shfl_xor(v[k], 32));
        if ((threadIdx.x & 63) < 16 && v[k] != 0ull) atomicMax(&slots[(int64_t)(P * 16 + col) * 16 + k], v[k]);
    }
}
template <typename T>
__global__ __launch_bounds__(256) void k_shared_norms(int n, int m, int NP, int MP, const T* __restrict__ Ax, const T* __restrict__ Px, const T* __restrict__ Aty,
                                                      const T* __restrict__ q, const T* __restrict__ x, const T* __restrict__ xp, const T* __restrict__ z,
                                                      const T* __restrict__ zp, unsigned long long* __restrict__ slots) {
    shared_norms_body<T, false>(n, m, NP, MP, Ax, Px, Aty, q, x, xp, z, zp, slots, nullptr, nullptr);
}
template <typename T>
__global__ __launch_bounds__(256) void k_shared_norms_equil(int n, int m, int NP, int MP, const T* __restrict__ Ax, const T* __restrict__ Px,
                                                            const T* __restrict__ Aty, const T* __restrict__ q, const T* __restrict__ x, const T* __restrict__ xp,
                                                            const T* __restrict__ z, const T* __restrict__ zp, unsigned long long* __restrict__ slots,
                                                            const int* __restrict__ kd, const int* __restrict__ ke) {
    shared_norms_body<T, true>(n, m, NP, MP, Ax, Px, Aty, q, x, xp, z, zp, slots, kd, ke);
}

// ---- Ruiz equilibration with exact powers of two (qps_set_shared_equilibration) ------------------------------------------------------------------------------
__device__ __forceinline__ double eq_ldexp(double v, int k) { return ldexp(v, k); }
__device__ __forceinline__ float eq_ldexp(float v, int k) { return ldexpf(v, k); }

// out[r] = 2^kr[r] max_c |M[r][c]| 2^kc[c] in double for a row-major rows x K matrix (ld = K, a multiple of 64): one wave per row, 16 bytes per lane and load,
// the wave's maximum on the VALU (wave_reduce.h).  Every norm is one wave's own reduction: no atomics, nothing crosses a workgroup, the result does not depend
// on the launch geometry.  The matrix is read through the exponents and never rewritten between passes (a power of two moves a double exactly).
// RANGE: also lo[r] = the smallest non-zero scaled magnitude of the row (+Inf for an empty row), for the range check before the matrices are touched.
template <typename T, bool RANGE>
__global__ __launch_bounds__(256) void k_equil_rownorm(const T* __restrict__ M, int rows, int K, const int* __restrict__ kr, const int* __restrict__ kc,
                                                       double* __restrict__ out, double* __restrict__ lo) {
    constexpr int VN = VecOf<T>::N;
    typedef T NV __attribute__((ext_vector_type(VN)));
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;                                         // wave-uniform
    const T* row = M + (int64_t)r * K;
    double hi = 0.0, mn = INFINITY;
    for (int c = lane * VN; c < K; c += 64 * VN) {                 // K is a multiple of 64, hence of VN: c < K means c + VN <= K
        const NV a = *reinterpret_cast<const NV*>(row + c);
#pragma unroll
        for (int j = 0; j < VN; ++j) {
            const double s = ldexp(fabs((double)a[j]), kc[c + j]);
            hi = fmax(hi, s);
            if (RANGE && s > 0.0) mn = fmin(mn, s);
        }
    }
    hi = wave_max_all_nonneg(hi);
    if (RANGE) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) mn = fmin(mn, __shfl_xor(mn, o));
    }
    if (lane == 0) {
        out[r] = ldexp(hi, kr[r]);
        if (RANGE) lo[r] = ldexp(mn, kr[r]);
    }
}

// k[i] = clamp(k[i] + step(max(a[i], b[i])), -13, 13) with step(v) = -floor(e / 2) for v = f 2^e, f in [0.5, 1) -- the power of two nearest to 1 / sqrt(v) on
// a log scale -- and step(0) = 0 (an empty or padding row).  b may be NULL.  13: OSQP's [1e-4, 1e4].
__global__ void k_equil_update(int len, const double* __restrict__ a, const double* __restrict__ b, int* __restrict__ k) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= len) return;
    double v = a[i];
    if (b) v = fmax(v, b[i]);
    int step = 0;
    if (v > 0.0) { int e; (void)frexp(v, &e); step = -(e >> 1); }   // >> on a negative int: arithmetic, i.e. floor
    k[i] = max(-13, min(13, k[i] + step));
}

// M[r][c] *= 2^(sign (kr[r] + kc[c])) in place, 16 bytes per lane (rows x cols, ld = cols, a multiple of VN)
template <typename T>
__global__ __launch_bounds__(256) void k_scale_two_sided(T* __restrict__ M, int64_t vecs, int vpr, const int* __restrict__ kr, const int* __restrict__ kc, int sign) {
    constexpr int VN = VecOf<T>::N;
    typedef T NV __attribute__((ext_vector_type(VN)));
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= vecs) return;
    const int r = (int)(i / vpr), c = (int)(i % vpr) * VN, er = kr[r];
    NV a = reinterpret_cast<NV*>(M)[i];
#pragma unroll
    for (int j = 0; j < VN; ++j) a[j] = eq_ldexp(a[j], sign * (er + kc[c + j]));
    reinterpret_cast<NV*>(M)[i] = a;
}

// dst[panel][row][16] = src[panel][row][16] 2^(sign k[row]), 16 bytes per lane (VN neighbouring columns of one row); dst may be src.  +-Inf stays +-Inf.
template <typename T>
__global__ __launch_bounds__(256) void k_panel_rowscale(const T* src, const int* __restrict__ k, int sign, int rowsP, int64_t vecs, T* dst) {
    constexpr int VN = VecOf<T>::N;
    typedef T NV __attribute__((ext_vector_type(VN)));
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= vecs) return;
    const int e = sign * k[(int)(((i * VN) >> 4) % rowsP)];
    NV a = reinterpret_cast<const NV*>(src)[i];
#pragma unroll
    for (int j = 0; j < VN; ++j) a[j] = eq_ldexp(a[j], e);
    reinterpret_cast<NV*>(dst)[i] = a;
}

// v[i] *= 2^(sign e[i]): the value arrays of the sparse handle (the factor's [P; A] values, the CSR copies of the check), exponent per entry from the pattern
template <typename T>
__global__ __launch_bounds__(256) void k_scale_entries(T* __restrict__ v, const int* __restrict__ e, int sign, int64_t cnt) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < cnt) v[i] = eq_ldexp(v[i], sign * e[i]);
}

// dst[k] = 2^e[k] (T) src[map[k]]: one value array of a sparse handle rebuilt from the caller's canonical CSC values (qps_update_shared_matrices_csc).  The value
// is rounded to T first and scaled afterwards, as creation followed by k_scale_entries does, so both ways give the same bits.  MAP false: dst is in CSC order
// itself (src[k]); EXP false: no scaling.  map[k] < cnt by construction (a permutation of the positions of one matrix).
template <typename T, bool MAP, bool EXP>
__global__ __launch_bounds__(REFRESH_VALUES_THREADS) void k_refresh_values(const double* __restrict__ src, const int* __restrict__ map, const int* __restrict__ e,
                                                                           int64_t cnt, T* __restrict__ dst) {
    const int64_t k = (int64_t)blockIdx.x * REFRESH_VALUES_THREADS + threadIdx.x;
    if (k >= cnt) return;
    const T v = (T)src[MAP ? (int64_t)map[k] : k];
    dst[k] = EXP ? eq_ldexp(v, e[k]) : v;
}

// The tests of qps_update_shared_values on the staged values of one matrix (validate_values in qps_kernels.h: the keys and what they mean).  Reads src and the
// index arrays, writes nothing but the keys.  A lane past cnt stays in the kernel with neutral keys: the wave reductions want every lane.  The finite and the
// symmetric key reduce only in a wave that has something to report (a wave-uniform branch); SYM false / EXP false: that test is not compiled in.
template <typename T, bool SYM, bool EXP>
__global__ __launch_bounds__(VALIDATE_VALUES_THREADS) void k_validate_values(const double* __restrict__ src, int64_t cnt, const int* __restrict__ partner,
                                                                             const int* __restrict__ cp, const int* __restrict__ ri, int ncols,
                                                                             const int* __restrict__ e, unsigned long long* __restrict__ verdict) {
    constexpr int WAVES = VALIDATE_VALUES_THREADS / 64;
    __shared__ unsigned long long part[VALIDATE_VERDICT_KEYS][WAVES];
    const int64_t k = (int64_t)blockIdx.x * VALIDATE_VALUES_THREADS + threadIdx.x;
    const bool in = k < cnt;
    const double v = in ? src[k] : 0.0;
    unsigned long long key[VALIDATE_VERDICT_KEYS] = {0, 0, 0, 0};
    const bool nonfinite = !(fabs(v) <= 1.7976931348623157e308);
    if (__ballot(nonfinite)) key[0] = wave_max_all_key(nonfinite ? ~0ull - (unsigned long long)k : 0ull);
    if (SYM) {
        bool off = false;
        if (in) { const int p = partner[k]; off = p >= 0 ? v != src[p] : v != 0.0; }   // on the doubles, tolerance 0; -0.0 == 0.0
        if (__ballot(off)) {
            unsigned long long c = 0;
            if (off) {
                int lo = 0, hi = ncols;                                                 // the column of entry k: cp[lo] <= k < cp[lo + 1] (cp[ncols] = cnt > k)
                while (hi - lo > 1) { const int mid = lo + (hi - lo) / 2; if ((int64_t)cp[mid] <= k) lo = mid; else hi = mid; }
                c = ~0ull - (unsigned long long)min(lo, ri[k]);
            }
            key[1] = wave_max_all_key(c);
        }
    }
    if (EXP) {
        const double a = in ? ldexp(fabs((double)(T)v), e[k]) : 0.0;                    // equil_range_add, entry for entry
        const unsigned long long bits = (unsigned long long)__double_as_longlong(a);
        key[2] = wave_max_all_key(bits);
        key[3] = wave_max_all_key(a > 0.0 ? ~0ull - bits : 0ull);
    }
    if ((threadIdx.x & 63) == 0)
        for (int q = 0; q < VALIDATE_VERDICT_KEYS; ++q) part[q][threadIdx.x >> 6] = key[q];
    __syncthreads();
    if (threadIdx.x < VALIDATE_VERDICT_KEYS) {
        unsigned long long best = 0;
        for (int w = 0; w < WAVES; ++w) best = key_max(best, part[threadIdx.x][w]);
        if (best) atomicMax(verdict + threadIdx.x, best);
    }
}

__device__ __forceinline__ double sh_jmax(double a, double b) { return (isnan(a) || isnan(b)) ? (double)NAN : (a > b ? a : b); }

// the decision of k_check_decide for every active column (fixed rho: the proposal stays rho); res: 8 doubles per column
__global__ void k_shared_decide(int cols, const unsigned long long* __restrict__ slots, double* __restrict__ res, const int* __restrict__ active,
                                double epsAbs, double epsRel, double epsAdmm, double rho) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= cols || !active[b]) return;
    slots += (int64_t)b * 16; res += (int64_t)b * 8;
    double nv[9];
    for (int k = 0; k < 9; ++k) nv[k] = __longlong_as_double((long long)slots[k]);
    const double normResPrim = nv[0], normResDual = nv[1];                 // :85-86
    const double maxNormPrim = sh_jmax(nv[2], nv[3]);                       // :88
    const double maxNormDual = sh_jmax(sh_jmax(nv[4], nv[5]), nv[6]);       // :89
    const double epsPrim = epsAbs + epsRel * maxNormPrim;                   // :99
    const double epsDual = epsAbs + epsRel * maxNormDual;                   // :100
    int flag = 1;
    if ((normResPrim < epsPrim) && (normResDual < epsDual)) flag = 3;       // :102-104
    if ((nv[7] <= epsAdmm) && (nv[8] <= epsAdmm)) flag = 2;                 // :105-107 (not else)
    res[0] = normResPrim; res[1] = normResDual; res[2] = maxNormPrim; res[3] = maxNormDual;
    res[4] = rho; res[5] = (double)flag; res[6] = nv[7]; res[7] = nv[8];
}

// ---- infeasibility certificates (qps_set_shared_infeasibility; OSQP 3.4): three launches at a check, none in the iteration -----------------------------------
// dx = x - xp (n rows) and dyh = the projection of y - yp onto the polar of the recession cone of [l, u] (m rows; yp = y before this iteration's row update), for
// the columns of the active mask: a column that stopped keeps the differences of its own stopping check, padding rows and columns keep their zeros.  Differences
// are formed in T, as the check forms its own.  The projection keeps a NaN (d > 0 ? 0 : d), so a NaN difference reaches the norm and no certificate is issued.
// With equilibration the panels hold the scaled iterates and so do dx and dyh: a positive row scale changes neither a sign nor which bound is infinite.
template <typename T>
__global__ __launch_bounds__(256) void k_shared_deltas(int n, int m, int NP, int MP, const T* __restrict__ x, const T* __restrict__ xp, const T* __restrict__ y,
                                                       const T* __restrict__ yp, const T* __restrict__ l, const T* __restrict__ u, const int* __restrict__ active,
                                                       T* __restrict__ dx, T* __restrict__ dyh) {
    const int P = blockIdx.y, col = threadIdx.x & 15, rl = threadIdx.x >> 4;
    if (!active[P * 16 + col]) return;
    const int64_t on = (int64_t)P * NP * 16 + col, om = (int64_t)P * MP * 16 + col;
    for (int r = blockIdx.x * 16 + rl; r < max(n, m); r += gridDim.x * 16) {
        if (r < m) {
            const int64_t i = om + (int64_t)r * 16;
            const T d = y[i] - yp[i];
            const bool lo_inf = l[i] == -(T)INFINITY, hi_inf = u[i] == (T)INFINITY;
            dyh[i] = (lo_inf && hi_inf) ? T(0) : hi_inf ? (d > T(0) ? T(0) : d) : lo_inf ? (d < T(0) ? T(0) : d) : d;
        }
        if (r < n) {
            const int64_t i = on + (int64_t)r * 16;
            dx[i] = x[i] - xp[i];
        }
    }
}

// The seven figures of the two tests, per column, over the rows of one workgroup: part[(column * gridDim.x + blockIdx.x) * 8 + k], k =
//   0 ||dyh||  1 ||A'dyh||  2 S = sum_{dyh_i > 0} u_i dyh_i + sum_{dyh_i < 0} l_i dyh_i  3 ||dx||  4 ||P dx||  5 q'dx
//   6 the largest violation of the sign test on A dx: max(0, (A dx)_i over rows with a finite u_i, -(A dx)_i over rows with a finite l_i)
// all inf-norms, in the caller's units (EQ: E on dyh, D on dx, D^-1 on A'dyh and P dx, E^-1 on A dx -- exact powers of two, in double; the two sums are invariant
// under the scaling and are taken on the stored panels).  Norms travel as the bit patterns of non-negative doubles, so a NaN wins every maximum (k_shared_norms).
// The sums: every term is formed and added in double; a thread adds its rows in row order, the 16 threads of a column meet through two shuffles and the waves
// through LDS in wave order, and k_shared_cert_decide adds the workgroups in index order -- an order fixed by n, m and the launch geometry (shared_cert_blocks:
// n and m only), never by `count` or the column's position.  No atomics, no scratch.  Entries with dyh_i = 0 add nothing, so 0 * Inf never arises; dyh_i > 0
// implies a finite u_i and dyh_i < 0 a finite l_i by the projection.
template <typename T, bool EQ>
__global__ __launch_bounds__(256) void k_shared_cert_partial(int n, int m, int NP, int MP, const T* __restrict__ dx, const T* __restrict__ dyh,
                                                             const T* __restrict__ Adx, const T* __restrict__ Pdx, const T* __restrict__ Atdy,
                                                             const T* __restrict__ q, const T* __restrict__ l, const T* __restrict__ u,
                                                             const int* __restrict__ active, const int* __restrict__ kd, const int* __restrict__ ke,
                                                             double* __restrict__ part) {
    __shared__ double red[4][16][8];
    const int P = blockIdx.y, col = threadIdx.x & 15, rl = threadIdx.x >> 4, wv = threadIdx.x >> 6;
    const bool act = active[P * 16 + col] != 0;
    const int64_t on = (int64_t)P * NP * 16 + col, om = (int64_t)P * MP * 16 + col;
    unsigned long long v[5] = {0ull, 0ull, 0ull, 0ull, 0ull};   // ||dyh||, ||A'dyh||, ||dx||, ||P dx||, violation
    double S = 0.0, qd = 0.0;
    for (int r = blockIdx.x * 16 + rl; act && r < max(n, m); r += gridDim.x * 16) {
        if (r < m) {
            const int64_t i = om + (int64_t)r * 16;
            const T dv = dyh[i], lo = l[i], hi = u[i];
            const int s = EQ ? ke[r] : 0;
            v[0] = sh_umax(v[0], sh_absbits(EQ ? ldexp((double)dv, s) : (double)dv));
            if (dv > T(0)) S += (double)hi * (double)dv;
            else if (dv < T(0)) S += (double)lo * (double)dv;
            const double a = EQ ? ldexp((double)Adx[i], -s) : (double)Adx[i];
            if (hi != (T)INFINITY && !(a <= 0.0)) v[4] = sh_umax(v[4], sh_absbits(a));      // (a NaN counts as a violation)
            if (lo != -(T)INFINITY && !(a >= 0.0)) v[4] = sh_umax(v[4], sh_absbits(a));
        }
        if (r < n) {
            const int64_t i = on + (int64_t)r * 16;
            const T d = dx[i];
            const int s = EQ ? kd[r] : 0;
            v[2] = sh_umax(v[2], sh_absbits(EQ ? ldexp((double)d, s) : (double)d));
            v[3] = sh_umax(v[3], sh_absbits(EQ ? ldexp((double)Pdx[i], -s) : (double)Pdx[i]));
            v[1] = sh_umax(v[1], sh_absbits(EQ ? ldexp((double)Atdy[i], -s) : (double)Atdy[i]));
            qd += (double)q[i] * (double)d;
        }
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        v[k] = sh_umax(v[k], __shfl_xor(v[k], 16));
        v[k] = sh_umax(v[k], __shfl_xor(v[k], 32));
    }
    S += __shfl_xor(S, 16); S += __shfl_xor(S, 32);       // a + b is the same double on both lanes of a pair
    qd += __shfl_xor(qd, 16); qd += __shfl_xor(qd, 32);
    if ((threadIdx.x & 63) < 16) {
        double* o = red[wv][col];
        o[0] = __longlong_as_double((long long)v[0]); o[1] = __longlong_as_double((long long)v[1]); o[2] = S;
        o[3] = __longlong_as_double((long long)v[2]); o[4] = __longlong_as_double((long long)v[3]); o[5] = qd;
        o[6] = __longlong_as_double((long long)v[4]); o[7] = 0.0;
    }
    __syncthreads();
    if (threadIdx.x < 16 && act) {
        double o[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = red[0][col][k];
        for (int ww = 1; ww < 4; ++ww)
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const double t = red[ww][col][k];
                if (k == 2 || k == 5 || k == 7) o[k] += t;
                else o[k] = __longlong_as_double((long long)sh_umax((unsigned long long)__double_as_longlong(o[k]), (unsigned long long)__double_as_longlong(t)));
            }
        double* dst = part + ((int64_t)(P * 16 + col) * gridDim.x + blockIdx.x) * 8;
#pragma unroll
        for (int k = 0; k < 8; ++k) dst[k] = o[k];
    }
}

// The two tests for every column that is still running and that k_shared_decide left at flag 1 (flags 2 and 3 win): res[5] becomes 4 (primal infeasible) or 5
// (dual infeasible, tested only when the primal test failed), so the flags travel in the read-back the check makes anyway.  epsP / epsD = 0: that test is off.
// Every comparison with a NaN operand is false: no certificate.
__global__ void k_shared_cert_decide(int cols, int nblk, const double* __restrict__ part, double* __restrict__ res, const int* __restrict__ active, double epsP,
                                     double epsD) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= cols || !active[b]) return;
    res += (int64_t)b * 8;
    if (res[5] != 1.0) return;
    part += (int64_t)b * nblk * 8;
    double o[8];
    for (int k = 0; k < 8; ++k) o[k] = part[k];
    for (int j = 1; j < nblk; ++j)
        for (int k = 0; k < 8; ++k) {
            const double t = part[j * 8 + k];
            if (k == 2 || k == 5 || k == 7) o[k] += t;
            else o[k] = __longlong_as_double((long long)sh_umax((unsigned long long)__double_as_longlong(o[k]), (unsigned long long)__double_as_longlong(t)));
        }
    const double N = o[0], At = o[1], S = o[2], M = o[3], Pn = o[4], qd = o[5], V = o[6];
    const bool prim = (epsP > 0.0) && (N > epsP) && (S < -epsP * N) && (At < epsP * N);
    const bool dual = !prim && (epsD > 0.0) && (M > epsD) && (qd < -epsD * M) && (Pn < epsD * M) && (V < epsD * M);
    if (prim) res[5] = 4.0;
    else if (dual) res[5] = 5.0;
}

// host layout [count][len] doubles <-> panels [panel][rowsP][16] of T
template <typename T>
__global__ void k_to_panels(const double* __restrict__ src, int count, int len, int rowsP, T* __restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)count * len) return;
    const int b = (int)(i / len), r = (int)(i % len);
    dst[((int64_t)(b >> 4) * rowsP + r) * 16 + (b & 15)] = (T)src[i];
}
template <typename T>
__global__ void k_from_panels(const T* __restrict__ src, int count, int len, int rowsP, double* __restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)count * len) return;
    const int b = (int)(i / len), r = (int)(i % len);
    dst[i] = (double)src[((int64_t)(b >> 4) * rowsP + r) * 16 + (b & 15)];
}

// dst (cols x rows, ld ldd) = src' (rows x cols, ld lds); rows, cols multiples of 32
template <typename T>
__global__ __launch_bounds__(256) void k_transpose(const T* __restrict__ src, int64_t lds, T* __restrict__ dst, int64_t ldd) {
    __shared__ T tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
#pragma unroll
    for (int k = 0; k < 4; ++k) tile[ty + 8 * k][tx] = src[(int64_t)(r0 + ty + 8 * k) * lds + c0 + tx];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) dst[(int64_t)(c0 + ty + 8 * k) * ldd + r0 + tx] = tile[tx][ty + 8 * k];
}

// dst = diag(scale) src, 16 bytes per lane
template <typename T>
__global__ __launch_bounds__(256) void k_scale_rows(const T* __restrict__ src, const T* __restrict__ scale, int64_t vecs, int vpr, T* __restrict__ dst) {
    typedef T NV __attribute__((ext_vector_type(VecOf<T>::N)));
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= vecs) return;
    reinterpret_cast<NV*>(dst)[i] = reinterpret_cast<const NV*>(src)[i] * scale[i / vpr];
}

// w = rho z - y over [panel][MP][16] after a switch of the family rho (qps_set_shared_adaptive_rho): the expression of the EPI == 3 / EPI == 4 epilogues with
// the new rho, so that the next right-hand side reads what the row update would have left behind.  16 bytes per lane (VN neighbouring columns of one row);
// a stopped column keeps its w.  SCALED: rho_i of the row from rho_row.
template <typename T, bool SCALED>
__global__ __launch_bounds__(256) void k_panel_w(const T* __restrict__ z, const T* __restrict__ y, const int* __restrict__ active, const T* __restrict__ rho_row,
                                                 T rho, int MP, int64_t vecs, T* __restrict__ w) {
    constexpr int VN = VecOf<T>::N;
    typedef T NV __attribute__((ext_vector_type(VN)));
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= vecs) return;
    const int64_t e = i * VN;                                   // first element: (panel, row, column) = (e / (16 MP), e / 16 % MP, e % 16)
    const int P = (int)(e / ((int64_t)MP * 16)), row = (int)((e >> 4) % MP), col = (int)(e & 15);
    const T rr = SCALED ? rho_row[row] : rho;
    const NV zv = reinterpret_cast<const NV*>(z)[i], yv = reinterpret_cast<const NV*>(y)[i];
    NV wv = reinterpret_cast<const NV*>(w)[i];
#pragma unroll
    for (int j = 0; j < VN; ++j) {
        const T zn = zv[j], yn = yv[j];
        if (active[P * 16 + col + j]) wv[j] = panel_w_of(rr, zn, yn);
    }
    reinterpret_cast<NV*>(w)[i] = wv;
}

template <typename T, int TRI, int EPI, int PB, int SH_NW, bool STG>
void panel_launch(hipStream_t st, const PanelArgs<T>& a) {
    const dim3 grid((a.rows / 16) * ((a.npanel + PB - 1) / PB)), block(SH_NW * 64);
    if (g_launch_timing.start) {   // profiled launch: the dispatch's own timestamps (qps_kernels.h)
        const LaunchTiming lt = g_launch_timing;
        g_launch_timing = LaunchTiming();
        hipExtLaunchKernelGGL((k_panel<T, TRI, EPI, PB, SH_NW, STG>), grid, block, 0, st, lt.start, lt.stop, 0, a);
        return;
    }
    hipLaunchKernelGGL((k_panel<T, TRI, EPI, PB, SH_NW, STG>), grid, block, 0, st, a);
}
template <typename T, int TRI, int EPI>
void panel_shape(hipStream_t st, const PanelArgs<T>& a) {
    // The shape of the launch depends on the MATRIX only, so a column sees the same summation order whatever the batch around it is.
    if (shared_panel_small(a.rows, a.K, sizeof(T))) { panel_launch<T, TRI, EPI, 1, 16, false>(st, a); return; }
    if (a.npanel >= 2) panel_launch<T, TRI, EPI, 2, 8, true>(st, a); else panel_launch<T, TRI, EPI, 1, 8, true>(st, a);
}

}  // namespace

// Matrices of at most 32 MiB stay in L2 / Infinity Cache between launches: the launch is then bound by the chain of dependent loads of a wave, not
// by bytes -- one panel per workgroup (twice the workgroups, the matrix re-read from cache per panel) and 16 waves per workgroup halve that chain.
bool shared_panel_small(int rows, int K, size_t elem) { return (size_t)rows * (size_t)K * elem <= ((size_t)32 << 20); }

template <typename T>
void shared_panel(hipStream_t st, SharedPanelOp op, const PanelArgs<T>& a) {
    switch (op) {
        case SharedPanelOp::product: panel_shape<T, 0, 0>(st, a); break;
        case SharedPanelOp::rhs: panel_shape<T, 0, 1>(st, a); break;
        case SharedPanelOp::forward: panel_shape<T, 1, 0>(st, a); break;
        case SharedPanelOp::backward: panel_shape<T, 2, 0>(st, a); break;
        case SharedPanelOp::backward_x: panel_shape<T, 2, 2>(st, a); break;
        case SharedPanelOp::rows_zy: panel_shape<T, 0, 3>(st, a); break;
        case SharedPanelOp::rows_zy_scaled: panel_shape<T, 0, 4>(st, a); break;
        case SharedPanelOp::start_z: panel_shape<T, 0, 5>(st, a); break;
    }
}

template <typename T>
void shared_check(hipStream_t st, int n, int m, int NP, int MP, int npanel, const T* Ax, const T* Px, const T* Aty, const T* q, const T* x, const T* xp,
                  const T* z, const T* zp, unsigned long long* slots, double* res_dev, const int* active, double epsAbs, double epsRel, double epsAdmm,
                  double rho, const int* kd, const int* ke) {
    const int blocks = std::max(1, std::min((std::max(n, m) + 15) / 16, 256));
    if (kd) hipLaunchKernelGGL((k_shared_norms_equil<T>), dim3(blocks, npanel), dim3(256), 0, st, n, m, NP, MP, Ax, Px, Aty, q, x, xp, z, zp, slots, kd, ke);
    else hipLaunchKernelGGL((k_shared_norms<T>), dim3(blocks, npanel), dim3(256), 0, st, n, m, NP, MP, Ax, Px, Aty, q, x, xp, z, zp, slots);
    hipLaunchKernelGGL(k_shared_decide, dim3((npanel * 16 + 63) / 64), dim3(64), 0, st, npanel * 16, slots, res_dev, active, epsAbs, epsRel, epsAdmm, rho);
}

// workgroups per panel of the certificate sums: from n and m only, so that the summation order of a column never depends on the batch around it
int shared_cert_blocks(int n, int m) { return std::max(1, std::min((std::max(n, m) + 255) / 256, 64)); }

template <typename T>
void shared_deltas(hipStream_t st, int n, int m, int NP, int MP, int npanel, const T* x, const T* xp, const T* y, const T* yp, const T* l, const T* u,
                   const int* active, T* dx, T* dyh) {
    const int blocks = std::max(1, std::min((std::max(n, m) + 15) / 16, 256));
    hipLaunchKernelGGL((k_shared_deltas<T>), dim3(blocks, npanel), dim3(256), 0, st, n, m, NP, MP, x, xp, y, yp, l, u, active, dx, dyh);
}
template <typename T>
void shared_certificates(hipStream_t st, int n, int m, int NP, int MP, int npanel, const T* dx, const T* dyh, const T* Adx, const T* Pdx, const T* Atdy,
                         const T* q, const T* l, const T* u, const int* active, const int* kd, const int* ke, double* part, double* res_dev, double epsP,
                         double epsD) {
    const int nblk = shared_cert_blocks(n, m);
    if (kd) hipLaunchKernelGGL((k_shared_cert_partial<T, true>), dim3(nblk, npanel), dim3(256), 0, st, n, m, NP, MP, dx, dyh, Adx, Pdx, Atdy, q, l, u, active, kd, ke, part);
    else hipLaunchKernelGGL((k_shared_cert_partial<T, false>), dim3(nblk, npanel), dim3(256), 0, st, n, m, NP, MP, dx, dyh, Adx, Pdx, Atdy, q, l, u, active, kd, ke, part);
    hipLaunchKernelGGL(k_shared_cert_decide, dim3((npanel * 16 + 63) / 64), dim3(64), 0, st, npanel * 16, nblk, part, res_dev, active, epsP, epsD);
}

template <typename T> void to_panels(hipStream_t st, const double* src, int count, int len, int rowsP, T* dst) {
    const int64_t total = (int64_t)count * len;
    if (total <= 0) return;
    hipLaunchKernelGGL((k_to_panels<T>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, src, count, len, rowsP, dst);
}
template <typename T> void from_panels(hipStream_t st, const T* src, int count, int len, int rowsP, double* dst) {
    const int64_t total = (int64_t)count * len;
    if (total <= 0) return;
    hipLaunchKernelGGL((k_from_panels<T>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, src, count, len, rowsP, dst);
}
template <typename T> void transpose_rowmajor(hipStream_t st, const T* src, int64_t lds, int rows, int cols, T* dst, int64_t ldd) {
    hipLaunchKernelGGL((k_transpose<T>), dim3(cols / 32, rows / 32), dim3(256), 0, st, src, lds, dst, ldd);
}

template <typename T> void panel_w(hipStream_t st, const T* z, const T* y, const int* active, const T* rho_row, T rho, int MP, int npanel, T* w) {
    const int64_t vecs = (int64_t)npanel * MP * 16 / VecOf<T>::N;
    if (vecs <= 0) return;
    const dim3 grid((unsigned)((vecs + 255) / 256)), block(256);
    if (rho_row) hipLaunchKernelGGL((k_panel_w<T, true>), grid, block, 0, st, z, y, active, rho_row, rho, MP, vecs, w);
    else hipLaunchKernelGGL((k_panel_w<T, false>), grid, block, 0, st, z, y, active, rho_row, rho, MP, vecs, w);
}

template <typename T> void scale_rows(hipStream_t st, const T* src, const T* scale, int rows, int cols, T* dst) {
    const int vpr = cols / VecOf<T>::N;
    const int64_t vecs = (int64_t)rows * vpr;
    if (vecs <= 0) return;
    hipLaunchKernelGGL((k_scale_rows<T>), dim3((unsigned)((vecs + 255) / 256)), dim3(256), 0, st, src, scale, vecs, vpr, dst);
}

template <typename T> void equil_rownorm(hipStream_t st, const T* M, int rows, int K, const int* kr, const int* kc, double* out, double* lo) {
    if (rows <= 0) return;
    const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
    if (lo) hipLaunchKernelGGL((k_equil_rownorm<T, true>), grid, block, 0, st, M, rows, K, kr, kc, out, lo);
    else hipLaunchKernelGGL((k_equil_rownorm<T, false>), grid, block, 0, st, M, rows, K, kr, kc, out, lo);
}
void equil_update(hipStream_t st, int len, const double* a, const double* b, int* k) {
    if (len > 0) hipLaunchKernelGGL(k_equil_update, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, st, len, a, b, k);
}
template <typename T> void scale_two_sided(hipStream_t st, T* M, int rows, int cols, const int* kr, const int* kc, int sign) {
    const int vpr = cols / VecOf<T>::N;
    const int64_t vecs = (int64_t)rows * vpr;
    if (vecs <= 0) return;
    hipLaunchKernelGGL((k_scale_two_sided<T>), dim3((unsigned)((vecs + 255) / 256)), dim3(256), 0, st, M, vecs, vpr, kr, kc, sign);
}
template <typename T> void panel_rowscale(hipStream_t st, const T* src, const int* k, int sign, int rowsP, int npanel, T* dst) {
    const int64_t vecs = (int64_t)npanel * rowsP * 16 / VecOf<T>::N;
    if (vecs <= 0) return;
    hipLaunchKernelGGL((k_panel_rowscale<T>), dim3((unsigned)((vecs + 255) / 256)), dim3(256), 0, st, src, k, sign, rowsP, vecs, dst);
}
template <typename T> void scale_entries(hipStream_t st, T* v, const int* e, int sign, int64_t cnt) {
    if (cnt <= 0) return;
    hipLaunchKernelGGL((k_scale_entries<T>), dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, v, e, sign, cnt);
}
template <typename T> void refresh_values(hipStream_t st, const double* src, const int* map, const int* e, int64_t cnt, T* dst) {
    if (cnt <= 0) return;
    const dim3 grid((unsigned)((cnt + REFRESH_VALUES_THREADS - 1) / REFRESH_VALUES_THREADS)), block(REFRESH_VALUES_THREADS);
    if (map && e) hipLaunchKernelGGL((k_refresh_values<T, true, true>), grid, block, 0, st, src, map, e, cnt, dst);
    else if (map) hipLaunchKernelGGL((k_refresh_values<T, true, false>), grid, block, 0, st, src, map, e, cnt, dst);
    else if (e) hipLaunchKernelGGL((k_refresh_values<T, false, true>), grid, block, 0, st, src, map, e, cnt, dst);
    else hipLaunchKernelGGL((k_refresh_values<T, false, false>), grid, block, 0, st, src, map, e, cnt, dst);
}
template <typename T>
void validate_values(hipStream_t st, const double* src, int64_t cnt, const int* partner, const int* cp, const int* ri, int ncols, const int* e,
                     unsigned long long* verdict) {
    if (cnt <= 0) return;
    const dim3 grid((unsigned)((cnt + VALIDATE_VALUES_THREADS - 1) / VALIDATE_VALUES_THREADS)), block(VALIDATE_VALUES_THREADS);
    if (partner && e) hipLaunchKernelGGL((k_validate_values<T, true, true>), grid, block, 0, st, src, cnt, partner, cp, ri, ncols, e, verdict);
    else if (partner) hipLaunchKernelGGL((k_validate_values<T, true, false>), grid, block, 0, st, src, cnt, partner, cp, ri, ncols, e, verdict);
    else if (e) hipLaunchKernelGGL((k_validate_values<T, false, true>), grid, block, 0, st, src, cnt, partner, cp, ri, ncols, e, verdict);
    else hipLaunchKernelGGL((k_validate_values<T, false, false>), grid, block, 0, st, src, cnt, partner, cp, ri, ncols, e, verdict);
}

#define INST(T)                                                                                                                         \
    template void validate_values<T>(hipStream_t, const double*, int64_t, const int*, const int*, const int*, int, const int*,          \
                                     unsigned long long*);                                                                              \
    template void equil_rownorm<T>(hipStream_t, const T*, int, int, const int*, const int*, double*, double*);                          \
    template void scale_two_sided<T>(hipStream_t, T*, int, int, const int*, const int*, int);                                           \
    template void panel_rowscale<T>(hipStream_t, const T*, const int*, int, int, int, T*);                                              \
    template void scale_entries<T>(hipStream_t, T*, const int*, int, int64_t);                                                          \
    template void refresh_values<T>(hipStream_t, const double*, const int*, const int*, int64_t, T*);                                   \
    template void scale_rows<T>(hipStream_t, const T*, const T*, int, int, T*);                                                         \
    template void panel_w<T>(hipStream_t, const T*, const T*, const int*, const T*, T, int, int, T*);                                   \
    template void shared_panel<T>(hipStream_t, SharedPanelOp, const PanelArgs<T>&);                                                     \
    template void shared_check<T>(hipStream_t, int, int, int, int, int, const T*, const T*, const T*, const T*, const T*, const T*,     \
                                  const T*, const T*, unsigned long long*, double*, const int*, double, double, double, double,          \
                                  const int*, const int*);                                                                              \
    template void shared_deltas<T>(hipStream_t, int, int, int, int, int, const T*, const T*, const T*, const T*, const T*, const T*,    \
                                   const int*, T*, T*);                                                                                 \
    template void shared_certificates<T>(hipStream_t, int, int, int, int, int, const T*, const T*, const T*, const T*, const T*,        \
                                         const T*, const T*, const T*, const int*, const int*, const int*, double*, double*, double,    \
                                         double);                                                                                       \
    template void to_panels<T>(hipStream_t, const double*, int, int, int, T*);                                                          \
    template void from_panels<T>(hipStream_t, const T*, int, int, int, double*);                                                        \
    template void transpose_rowmajor<T>(hipStream_t, const T*, int64_t, int, int, T*, int64_t);
INST(double)
INST(float)
#undef INST

}  // namespace qps
