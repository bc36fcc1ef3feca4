// k_csr_panel.hip -- out = M B for a plain CSR matrix M and 16-column panels B: the products of the convergence check of the sparse
// shared-matrix batch (A x, P x, A'y; SolveQuadraticProgram.jl:79-112 per column).
//
// One (matrix row, panel) per 16 SPR lanes (panel_strips.h); blockIdx.y = panel.  ci[k] and va[k] are loaded once for 16 QPs and B[ci[k]] is one
// contiguous line of 16 elements.  No atomics: a row's sum has one fixed order whatever the batch around it is.
#include "panel_strips.h"
#include "qps_kernels.h"

namespace qps {

namespace {

template <typename T, int SPR>
__global__ __launch_bounds__(PS_THREADS) void k_csr_panel(int rows, const int* __restrict__ rp, const int* __restrict__ ci, const T* __restrict__ va,
                                                           const T* __restrict__ B, int rowsB, T* __restrict__ out, int rowsOut) {
    const int r = blockIdx.x * (PS_THREADS / (16 * SPR)) + threadIdx.x / (16 * SPR), strip = (threadIdx.x >> 4) % SPR, col = threadIdx.x & 15;
    const bool valid = r < rows;
    const T* Bp = B + (int64_t)blockIdx.y * rowsB * 16 + col;
    T s = T(0);
    if (valid) s = strip_dot<T, SPR>(rp[r], rp[r + 1], strip, ci, va, [&](int i) { return Bp[(int64_t)i * 16]; });
    s = strips_sum<T, SPR>(s);
    if (valid && strip == 0) out[((int64_t)blockIdx.y * rowsOut + r) * 16 + col] = s;
}

template <typename T, int SPR>
void csr_panel_launch(hipStream_t st, const CsrPanelMatrix<T>& M, const T* B, int rowsB, T* out, int rowsOut, int npanel) {
    constexpr int RPB = PS_THREADS / (16 * SPR);
    hipLaunchKernelGGL((k_csr_panel<T, SPR>), dim3((unsigned)((M.rows + RPB - 1) / RPB), (unsigned)npanel), dim3(PS_THREADS), 0, st, M.rows, M.rp, M.ci, M.va, B,
                       rowsB, out, rowsOut);
}

}  // namespace

int csr_panel_spr(int64_t nnz, int rows) { return pick_panel_spr(nnz, rows); }

template <typename T>
void csr_panel(hipStream_t st, const CsrPanelMatrix<T>& M, const T* B, int rowsB, T* out, int rowsOut, int npanel) {
    if (M.rows <= 0 || npanel <= 0) return;
    if (M.spr == 1) csr_panel_launch<T, 1>(st, M, B, rowsB, out, rowsOut, npanel);
    else if (M.spr == 4) csr_panel_launch<T, 4>(st, M, B, rowsB, out, rowsOut, npanel);
    else csr_panel_launch<T, 16>(st, M, B, rowsB, out, rowsOut, npanel);
}

template void csr_panel<double>(hipStream_t, const CsrPanelMatrix<double>&, const double*, int, double*, int, int);
template void csr_panel<float>(hipStream_t, const CsrPanelMatrix<float>&, const float*, int, float*, int, int);

}  // namespace qps
