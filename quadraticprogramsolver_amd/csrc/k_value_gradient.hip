// k_value_gradient.hip -- the gradients of qps_adjoint_shared with respect to the stored values of P and A: a sampled outer product on a CSR pattern, summed
// over all columns of the batch.
//
//     out[k] = scale * sum over the columns c of  U[a][c] V[b][c] + W[b][c] Z[a][c],      a = rowof[k], b = ci[k]
//
// P (its CSR copy, which is the CSC order of a symmetric matrix in full storage): U = W = r_x, V = Z = x, scale = -1/2.  A (the CSR copy of A', whose rows are
// the columns of A, hence the canonical CSC order): a is the column j, b the row i, U = r_x, Z = x, V = y, W = r_lambda, scale = -1.
//
// A row of 16 lanes owns one entry at a time; lane c is column c of a panel.  The lane runs over the panels in order and accumulates in double (also on fp32
// handles), the 16 lanes are added by the fixed tree of row16_sum_last and lane 15 stores one double.  Per entry and panel the four loads are 16 consecutive T
// each: one coalesced request per row of lanes.  No atomics, no LDS: the result depends on neither the grid nor the zero padding columns of the last panel, and
// repeats bit for bit.  A wave stays whole through the reduction: the lanes of an entry past the end recompute the last entry and store nothing.
#include <algorithm>

#include "qps_kernels.h"
#include "wave_reduce.h"

namespace qps {

namespace {

// VG_UNROLL entries per row of lanes and trip: their index loads, then their 4 VG_UNROLL panel loads, are in flight together (the kernel waits on two dependent
// round trips per trip, whatever their number); entry i of a trip is base + 16 i + row, so that the index loads of a workgroup are consecutive
constexpr int VG_THREADS = 256, VG_ROWS = VG_THREADS / 16, VG_UNROLL = 4, VG_ENTRIES = VG_ROWS * VG_UNROLL, VG_MAX_BLOCKS = 1024;

template <typename T>
__global__ __launch_bounds__(VG_THREADS) void k_value_gradient(int nnz, const int* __restrict__ rowof, const int* __restrict__ ci, const T* __restrict__ U,
                                                               const T* __restrict__ Z, int rowsA, const T* __restrict__ V, const T* __restrict__ W, int rowsB,
                                                               int npanel, double scale, double* __restrict__ out) {
    const int col = threadIdx.x & 15, sub = threadIdx.x >> 4;
    for (int64_t base = (int64_t)blockIdx.x * VG_ENTRIES; base < nnz; base += (int64_t)gridDim.x * VG_ENTRIES) {   // the same trip count in every lane of the block
        int k[VG_UNROLL]; bool valid[VG_UNROLL]; double s[VG_UNROLL];
        const T *ua[VG_UNROLL], *za[VG_UNROLL], *vb[VG_UNROLL], *wb[VG_UNROLL];
#pragma unroll
        for (int i = 0; i < VG_UNROLL; ++i) {
            const int64_t e = base + i * VG_ROWS + sub;
            valid[i] = e < nnz;
            k[i] = valid[i] ? (int)e : nnz - 1;
            const int a = rowof[k[i]], b = ci[k[i]];
            ua[i] = U + (int64_t)a * 16 + col; za[i] = Z + (int64_t)a * 16 + col; vb[i] = V + (int64_t)b * 16 + col; wb[i] = W + (int64_t)b * 16 + col;
            s[i] = 0.0;
        }
        for (int p = 0; p < npanel; ++p) {
            const int64_t oa = (int64_t)p * rowsA * 16, ob = (int64_t)p * rowsB * 16;
#pragma unroll
            for (int i = 0; i < VG_UNROLL; ++i) s[i] += (double)ua[i][oa] * (double)vb[i][ob] + (double)wb[i][ob] * (double)za[i][oa];
        }
#pragma unroll
        for (int i = 0; i < VG_UNROLL; ++i) {
            const double t = row16_sum_last(s[i]);
            if (valid[i] && col == 15) out[k[i]] = scale * t;
        }
    }
}

}  // namespace

template <typename T>
void panel_value_gradient(hipStream_t st, int64_t nnz, const int* rowof, const int* ci, const T* U, const T* Z, int rowsA, const T* V, const T* W, int rowsB, int npanel,
                          double scale, double* out) {
    if (nnz <= 0 || npanel <= 0) return;
    const int64_t blocks = std::min<int64_t>(VG_MAX_BLOCKS, (nnz + VG_ENTRIES - 1) / VG_ENTRIES);
    hipLaunchKernelGGL((k_value_gradient<T>), dim3((unsigned)blocks), dim3(VG_THREADS), 0, st, (int)nnz, rowof, ci, U, Z, rowsA, V, W, rowsB, npanel, scale, out);
}

template void panel_value_gradient<double>(hipStream_t, int64_t, const int*, const int*, const double*, const double*, int, const double*, const double*, int, int, double,
                                           double*);
template void panel_value_gradient<float>(hipStream_t, int64_t, const int*, const int*, const float*, const float*, int, const float*, const float*, int, int, double,
                                          double*);

}  // namespace qps
