// panel_strips.h -- sparse row x 16-column panel: the gather loop the panel sweeps of k_ldl.hip and the CSR x panel product of
// k_csr_panel.hip share (device code, internal).
//
// One (row, panel) is worked on by SPR strips of 16 lanes (one DPP row each), SPR in {1, 4, 16}; lane % 16 is the QP column.  Strip s takes
// the entries k0 + s, k0 + s + SPR, ... of the row: every lane of a strip reads the same idx[k] and val[k] (one broadcast request) and
// its own column of the 16-wide line the index points at.  Four independent gathers are in flight per lane; their partial sums and then the
// strips are added in a fixed order that depends on the row's length and SPR only -- never on the panel or on how many panels there are.
#pragma once
#include <hip/hip_runtime.h>

namespace qps {

constexpr int PS_THREADS = 256;   // workgroup size of every strip kernel: 16, 4 or 1 rows per workgroup for SPR = 1, 4, 16

// xcol(i): the value of the lane's column in line i
template <typename T, int SPR, typename F>
__device__ __forceinline__ T strip_dot(int k0, int ke, int strip, const int* __restrict__ idx, const T* __restrict__ val, F&& xcol) {
    T s0 = T(0), s1 = T(0), s2 = T(0), s3 = T(0);
    int k = k0 + strip;
    for (; k + 3 * SPR < ke; k += 4 * SPR) {
        s0 += val[k] * xcol(idx[k]); s1 += val[k + SPR] * xcol(idx[k + SPR]);
        s2 += val[k + 2 * SPR] * xcol(idx[k + 2 * SPR]); s3 += val[k + 3 * SPR] * xcol(idx[k + 3 * SPR]);
    }
    for (; k < ke; k += SPR) s0 += val[k] * xcol(idx[k]);
    return (s0 + s1) + (s2 + s3);
}

// Sum of the SPR strips of a row, valid in strip 0.  Every lane of the workgroup must call it (wave shuffles; a barrier for SPR = 16).
// SPR = 4: the strips are the four DPP rows of one wave, ((p0 + p1) + (p2 + p3)).  SPR = 16: that sum per wave, then the four waves of the
// workgroup through LDS, (w0 + w1) + (w2 + w3).
template <typename T, int SPR>
__device__ __forceinline__ T strips_sum(T s) {
    if (SPR == 1) return s;
    s += __shfl_xor(s, 16);
    s += __shfl_xor(s, 32);
    if (SPR == 16) {
        __shared__ T wsum[4][16];
        const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
        if (lane < 16) wsum[w][lane] = s;
        __syncthreads();
        const int c = threadIdx.x & 15;
        s = (wsum[0][c] + wsum[1][c]) + (wsum[2][c] + wsum[3][c]);
    }
    return s;
}

// strips for rows of this mean length: a strip should find about eight entries (two rounds of four gathers) before it pays to split the row further
inline int pick_panel_spr(int64_t nnz, int rows) {
    if (rows <= 0) return 1;
    const double avg = (double)nnz / rows;
    return avg <= 8.0 ? 1 : (avg <= 64.0 ? 4 : 16);
}

}  // namespace qps
