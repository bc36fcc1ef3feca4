// qps_kernels.h -- host-callable launchers of the gfx950 kernels (internal; the public boundary is include/qps.h).
//
// Device data layout (dense path), all in HBM, T = double or float:
//   A   : m x n, ROW-major, leading dimension NP = roundup(n, 64), MP = roundup(m, 64) rows allocated, zero padded.
//   P   : n x n symmetric, row-major (== column-major), ld NP, zero padded.
//   S   : NP x NP "sweep matrix": lower triangle = W, upper triangle = W' where W is the Cholesky factor L of
//         M = P + sigma I + rho A'A with its nb x nb diagonal blocks replaced by their inverses.  Both triangular
//         sweeps are then row-dot-product GEMVs over S (forward reads c <= r, backward reads c >= r).
//   vectors of length n / m are allocated NP / MP long and zero padded.
#pragma once
#ifndef QPS_NT_SLABS
#define QPS_NT_SLABS 1   // non-temporal (write-through) stores for the per-workgroup slabs of the pass and sweep kernels
#endif
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <thread>

namespace qps {

// ---- per-device facts (qps_capi.hip).  A process may hold handles on several devices (include/qps.h:19), so nothing that
// describes or configures a DEVICE is cached in a plain function-local static: it is keyed by the device ordinal. ----------------------
constexpr int kMaxDevices = 64;
int current_device();                 // hipGetDevice (the entry points of a handle make its device current first)
int device_cu_count(int device);      // multiProcessorCount, asked once per ordinal
// Per-device one-time settings such as hipFuncSetAttribute(MaxDynamicSharedMemorySize): `once(dev, f)` runs f exactly once per device ordinal and returns,
// on EVERY calling thread, only after f has returned -- a second host thread (distinct handles may be driven from distinct threads, include/qps.h:19) must
// not launch the kernel before the attribute is in place (its launch with 144-160 KiB of dynamic LDS would fail).
struct PerDeviceOnce {
    std::atomic<unsigned char> state[kMaxDevices] = {};          // 0 not started, 1 running, 2 done
    template <typename F> void once(int dev, F&& f) {
        if (dev < 0 || dev >= kMaxDevices) { f(); return; }
        if (state[dev].load(std::memory_order_acquire) == 2) return;
        unsigned char expect = 0;
        if (state[dev].compare_exchange_strong(expect, 1, std::memory_order_acq_rel)) { f(); state[dev].store(2, std::memory_order_release); return; }
        while (state[dev].load(std::memory_order_acquire) != 2) std::this_thread::yield();
    }
};

// A launcher that finds a pending event pair here attaches it to its kernel dispatch (hipExtLaunchKernelGGL): the events then carry the
// kernel's own begin / end timestamps -- what rocprofv3 reports -- instead of bracketing the launch from outside (+3-4 us of
// launch gap and event handling).  Thread-local: handles may be driven from different host threads.
struct LaunchTiming { hipEvent_t start = nullptr, stop = nullptr; };
extern thread_local LaunchTiming g_launch_timing;


// Batched launches (BASELINE config 4: many independent QPs of one shape per GPU): blockIdx.y = QP index, element strides
// between consecutive QPs for the matrix / input-vector / output-vector operands, optional per-QP active mask.
// Default-constructed = the single-QP launch (count 1, no offsets).
struct BatchStride { int count = 1; int64_t mat = 0, vin = 0, vout = 0; const int* active = nullptr; };

template <typename T> struct VecOf;
template <> struct VecOf<double> { using type = double2; static constexpr int N = 2; };
template <> struct VecOf<float>  { using type = float4;  static constexpr int N = 4; };

// ---- loop kernels (k_loop.hip) -------------------------------------------------------------------------------
// out[r] = alpha * sum_{c in [c0,c1), tri} S[r][c] v[c] + beta * out0[r]   for r in [r0, r1); tri: 0 none, 1 c<=r, 2 c>=r
template <typename T>
void gemv_rows(hipStream_t st, const T* S, int64_t ld, const T* v, T* out, const T* out0, T alpha, T beta,
               int r0, int r1, int c0, int c1, int tri, BatchStride bs = BatchStride());

// part[t][c] = sum_{r in row tile t} S[r][c] * (ca*va[r] + cb*vb[r])  for c in [0, ncols); returns number of tiles
template <typename T>
int gemv_cols_partial(hipStream_t st, const T* S, int64_t ld, const T* va, const T* vb, T ca, T cb,
                      T* part, int64_t part_ld, int nrows, int ncols);
int gemv_cols_tiles(int nrows);

// out[c] = s0*a0[c] + s1*a1[c] + sum_{t<ntiles} part[t][c]
template <typename T>
void colsum(hipStream_t st, const T* part, int64_t part_ld, int ntiles, const T* a0, T s0, const T* a1, T s1,
            T* out, int ncols, BatchStride bs = BatchStride());   // bs.mat = stride between slab sets

// SolveQuadraticProgram.jl:56-61 fused: xp=x; x=alpha*xx+(1-alpha)*x; zp=z; z=clamp(...); y=y+rho*(...)
template <typename T>
void admm_update(hipStream_t st, int NP, int MP, const T* xx, const T* zz, T* x, T* xp, T* z, T* zp, T* y,
                 const T* l, const T* u, T alpha, T rho);

// SolveQuadraticProgram.jl:79-112: norms + decision.  Ax, Px, Aty are precomputed by GEMVs.  res = 16 doubles:
//  [0] resPrim [1] resDual [2] maxNormPrim [3] maxNormDual [4] rhorho [5] convFlag [6] dx [7] dz
struct CheckScalars { double epsAbs, epsRel, epsAdmm, rho, rhorho; int adptRho; int convFlag; };
template <typename T>
void check_convergence(hipStream_t st, int n, int m, const T* Ax, const T* Px, const T* Aty, const T* q, const T* x,
                       const T* xp, const T* z, const T* zp, unsigned long long* scratch /*>=16 u64 per QP*/, double* res_dev,
                       CheckScalars cs, int dual_only = 0, BatchStride bs = BatchStride(), const double* rho_arr = nullptr,
                       const double* rhorho_arr = nullptr);   // batched: bs.vin = n-vector stride, bs.vout = m-vector stride
// dual_only = 1: the primal-side slots (0,2,3,7,8) were already filled by the fused pass (k_pass.hip); scratch is not
// cleared and only the n-length norms are added before the decision.

// ---- fused single pass over A (k_pass.hip) -----------------------------------------------------------------------
// z~ = A x~, z/y update (SolveQuadraticProgram.jl:59-61), x_new = alpha x~ + (1-alpha) x_old (:57), slabs of
// A'(rho z_new - y_new) for the next right-hand side; check = true adds A x_new norms, slabs of A'y_new, |x_new-x_old|.
template <typename T> int apass_plan(int NP, int MP, int* rows_per_wg, int count = 1);   // slabs per QP (0: unsupported)
template <typename T> int apass_max_np();
// Batched form: blockIdx.y = QP; strides are MP*ld (A), NP (n-vectors), MP (m-vectors), slabs*part_ld (slabs), 16 (slots);
// rho_arr (double per QP) overrides the scalar rho; active masks finished QPs.
struct PassBatch { int count = 1; int slabs = 0; const double* rho_arr = nullptr; const int* active = nullptr; int pq_me = 0; };
template <typename T>
void apass(hipStream_t st, bool check, const T* A, int64_t ld, int NP, int MP, const T* xx, const T* x_old, T* x_new, T* z,
           T* y, const T* l, const T* u, T alpha, T rho, T* part, T* part2, int64_t part_ld, unsigned long long* slots,
           PassBatch pb = PassBatch());
// ProxQP.jl rows over G = [A; C] (k_pass_pq.hip): v = G x, slack/dual updates (ProxQP.jl:227-249) and the slabs of
// G'[rho b - y ; rho (d - s) - z] for the next right-hand side (:212-216) in one read of G.  Returns the slab count (0: unsupported).
template <typename T> int apass_proxqp_slabs(int NP, int MP);
// polishing (SolveQuadraticProgram.m:304-305): out_lam = mask (A vx) - delta mask vlam, slabs of A'(mask vlam); 0: unsupported shape
template <typename T>
int apass_kkt(hipStream_t st, const T* A, int64_t ld, int NP, int MP, const T* vx, const T* vlam, const T* mask, T delta, T* out_lam,
              T* part, int64_t part_ld);
template <typename T>
int apass_proxqp(hipStream_t st, const T* G, int64_t ld, int NP, int MP, int me, const T* x, T* x_scratch, T* slack, T* dual,
                 const T* g, T rho, T* part, int64_t part_ld);

// ---- whitened two-launch iteration of a dense fp64 handle on its cached factor (k_pass_w.hip) -------------------------------------
// B = A W' (MP x NP, ld, padded like A), G = W W' (lower triangle read), u = W t; the pass streams [B ; tril(G)] once: z~ = B u with the z / y row updates
// and a+ = alpha z~ + (1 - alpha) a (a = A x), slabs of B'(rho z - y), gd[r] = sum_{c <= r} G[r][c] u[c] and slabs of the strictly lower G'u;
// check = true adds slabs of B'y and the primal-side norms (slots 0, 2, 3, 8) from a+ and z+.  Every slab set has whitened_slabs() rows.
template <typename T> struct WhitenedPass {
    const T *B = nullptr, *G = nullptr; int64_t ld = 0; int NP = 0, MP = 0, rows_per_wg = 0;
    const T* u = nullptr; T *z = nullptr, *y = nullptr, *a = nullptr; const T *l = nullptr, *hi = nullptr;
    T alpha = T(0), rho = T(1);
    T *gd = nullptr, *slab_e = nullptr, *slab_g = nullptr, *slab_y = nullptr; int64_t part_ld = 0;
    unsigned long long* slots = nullptr;
};
// g = gd + sum slab_g, p_new = alpha g + (1 - alpha) p_old, u = sigma p_new - c + sum slab_e, with_bty: bty = sum slab_y; first: p_new = p_old, u = sigma p_old - c
template <typename T> struct WhitenedSum {
    const T *slab_e = nullptr, *slab_g = nullptr, *slab_y = nullptr; int64_t part_ld = 0; int ntiles = 0, ncols = 0, first = 0;
    const T *gd = nullptr, *p_old = nullptr, *c = nullptr; T *p_new = nullptr, *u = nullptr, *bty = nullptr;
    T alpha = T(0), sigma = T(0);
};
bool whitened_supported(int NP, int MP);
int whitened_slabs();
void whitened_pass(hipStream_t st, bool check, WhitenedPass<double> a);
void whitened_sum(hipStream_t st, bool with_bty, const WhitenedSum<double>& a);
// x = L pn, slots[7] = max |L (pn - po)|, aty = L bty over the lower triangle of L, read once
void whitened_lpass(hipStream_t st, const double* L, int64_t ld, int NP, const double* pn, const double* po, const double* bty, double* x, double* aty,
                    unsigned long long* slots);
void tril_copy(hipStream_t st, const double* S, double* D, int NP);   // D = lower triangle of S (NP x NP, ld NP), zeros above the diagonal

// ---- fused triangular sweeps (k_trsv.hip) -----------------------------------------------------------------------------
template <typename T> bool sweep_fused_supported(int NP);
// Both sweeps fused into one pass over the lower triangle (single inverted block): slabs of x~ = W' (W t); the caller adds
// the slabs with colsum().  bs.mat = stride between sweep matrices, bs.vin = stride of t, bs.vout = stride between the slab sets of two QPs.
template <typename T> int sweep_fused_slabs(int NP, int count = 1);
template <typename T>
int sweep_fused(hipStream_t st, const T* S, int64_t ld, int NP, const T* v, T* part, int64_t part_ld, BatchStride bs = BatchStride());

// ---- shared-matrix batch (k_shared.hip): many QPs on ONE P and ONE A, state in 16-column panels ------------------------------
// A length-R vector of `count` QPs is stored as panels [panel][rowsP][16]: QP b = column b % 16 of panel b / 16, rowsP = NP or MP, the column
// count padded to a multiple of 16 with columns that stay zero and inactive.  Every product of the loop is
//     out[panel][r][16] = sum_k Mat[r][k] * B[panel][k][16]          Mat row-major (ld), rows and K multiples of 64
// on the MFMA pipe (v_mfma_f64_16x16x4_f64 / v_mfma_f32_16x16x4_f32), the matrix streamed once for all panels of a launch (two panels per
// workgroup; more panels than that stream it once per pair, the pairs of one row tile side by side on one XCD), with the row-wise part of the
// iteration as its epilogue.
template <typename T> struct PanelArgs {
    const T* Mat = nullptr; int64_t ld = 0; int rows = 0, K = 0;
    const T* B = nullptr; int npanel = 0;
    T* out = nullptr;
    const T* q = nullptr; T *x = nullptr, *xp = nullptr;                                             // rhs, backward_x
    T *z = nullptr, *zp = nullptr, *y = nullptr, *w = nullptr; const T *l = nullptr, *u = nullptr;   // rows_zy
    const int* active = nullptr;                                                                     // one word per column (npanel * 16)
    T alpha = T(0), rho = T(1), sigma = T(0);
    const T *rho_row = nullptr, *rho1_row = nullptr;                                                 // rows_zy_scaled: rho_i and 1 / rho_i per matrix row (`rows` long)
};
enum class SharedPanelOp {
    product,      // out = Mat B                                                     (the check's A x, P x, A'y)
    rhs,          // out = sigma x - q + Mat B                                       LinearSystemSolvers.jl:134-136 with Mat = A', B = rho z - y
    forward,      // out = tril(Mat) B                                               forward sweep over the sweep matrix S (one inverted block)
    backward,     // out = triu(Mat) B                                               backward sweep alone (dense tail of the sparse shared batch)
    backward_x,   // out = triu(Mat) B; active columns: xp = x, x = alpha out + (1 - alpha) x      backward sweep + SolveQuadraticProgram.jl:56-57
    rows_zy,      // s = Mat B = z~; active columns: zp = z, z, y updated, w = rho z - y           SolveQuadraticProgram.jl:59-61
    rows_zy_scaled,  // rows_zy with rho read as diag(rho_i): row r takes rho_row[r] and rho1_row[r] in z, y and w (qps_set_shared_rho_scale)
    start_z          // s = Mat B = A x~; active columns: z = s, w = rho_i z - y (rho_i = rho_row[r], or rho when rho_row is NULL)     qps_set_shared_warm_start, mode 2
};
template <typename T> void shared_panel(hipStream_t st, SharedPanelOp op, const PanelArgs<T>& a);
bool shared_panel_small(int rows, int K, size_t elem);   // matrix small enough to stay cached: one panel and 16 waves per workgroup
// CheckConvergence per column (SolveQuadraticProgram.jl:79-112) on panels: slots = 16 u64 per column (zero-filled by the caller), res_dev = 8 doubles
// per column laid out as check_convergence's ([4] = rho: the shared batch runs a fixed rho)
template <typename T>
void shared_check(hipStream_t st, int n, int m, int NP, int MP, int npanel, const T* Ax, const T* Px, const T* Aty, const T* q, const T* x, const T* xp,
                  const T* z, const T* zp, unsigned long long* slots, double* res_dev, const int* active, double epsAbs, double epsRel, double epsAdmm,
                  double rho, const int* kd = nullptr, const int* ke = nullptr);
// kd / ke (both or neither; NP / MP ints): the panels hold iterates scaled by qps_set_shared_equilibration (D = 2^kd on the variables, E = 2^ke on the constraints) and
// the norms are taken of the unscaled quantities (OSQP 5.1) by a sibling of the norm kernel; without them the launch is the one above, argument for argument.
// Infeasibility certificates of the shared-matrix batches (qps_set_shared_infeasibility; OSQP 3.4), at a check and only while the option is on.  shared_deltas: for
// the active columns dx = x - xp (n rows) and dyh = the projection of y - yp onto the polar of the recession cone of [l, u] (m rows); other columns, padding rows
// and padding columns are left alone.  shared_certificates: Adx = A dx, Pdx = P dx, Atdy = A'dyh come from the check's product launches; per column the norms and
// the two double sums of the rule are reduced in a fixed order (part: 8 * 16 npanel * shared_cert_blocks(n, m) doubles) and a column that is active and stands at
// res_dev[8 b + 5] == 1 gets 4 (primal infeasible) or 5 (dual infeasible) there.  epsP / epsD = 0 leaves that test out.  kd / ke as for shared_check.
int shared_cert_blocks(int n, int m);
template <typename T>
void shared_deltas(hipStream_t st, int n, int m, int NP, int MP, int npanel, const T* x, const T* xp, const T* y, const T* yp, const T* l, const T* u,
                   const int* active, T* dx, T* dyh);
template <typename T>
void shared_certificates(hipStream_t st, int n, int m, int NP, int MP, int npanel, const T* dx, const T* dyh, const T* Adx, const T* Pdx, const T* Atdy,
                         const T* q, const T* l, const T* u, const int* active, const int* kd, const int* ke, double* part, double* res_dev, double epsP,
                         double epsD);
// Exact power-of-two Ruiz equilibration of the shared-matrix batches (k_shared.hip).  equil_rownorm: out[r] = 2^kr[r] max_c |M[r][c]| 2^kc[c] in double for a
// row-major rows x K matrix (ld = K, a multiple of 64); lo != NULL: also the smallest non-zero scaled magnitude per row (+Inf: none).  equil_update: k[i] =
// clamp(k[i] - floor(e / 2), -13, 13) for max(a[i], b[i]) = f 2^e, f in [0.5, 1) (0: k stays; b may be NULL).  scale_two_sided: M[r][c] *= 2^(sign (kr[r] + kc[c]))
// in place.  panel_rowscale: dst[panel][row][16] = src 2^(sign k[row]) (dst may be src).  scale_entries: v[i] *= 2^(sign e[i]).
template <typename T> void equil_rownorm(hipStream_t st, const T* M, int rows, int K, const int* kr, const int* kc, double* out, double* lo);
void equil_update(hipStream_t st, int len, const double* a, const double* b, int* k);
template <typename T> void scale_two_sided(hipStream_t st, T* M, int rows, int cols, const int* kr, const int* kc, int sign);
template <typename T> void panel_rowscale(hipStream_t st, const T* src, const int* k, int sign, int rowsP, int npanel, T* dst);
template <typename T> void scale_entries(hipStream_t st, T* v, const int* e, int sign, int64_t cnt);
// refresh_values: dst[k] = 2^e[k] (T) src[map[k]] for k < cnt -- a value array of a sparse shared-matrix batch rebuilt from canonical CSC values in double
// (qps_update_shared_matrices_csc); rounded to T first, scaled afterwards.  map == NULL: src[k]; e == NULL: no scaling.  One entry per lane.
constexpr int REFRESH_VALUES_THREADS = 256;
template <typename T> void refresh_values(hipStream_t st, const double* src, const int* map, const int* e, int64_t cnt, T* dst);
// validate_values: what has to hold for the staged canonical CSC values src[0, cnt) of one matrix before a values-only update may touch the handle
// (qps_update_shared_values), decided on the device.  It reads the staging and the index arrays only and writes VALIDATE_VERDICT_KEYS keys into `verdict`
// (zeroed by the caller; every key is a maximum over the entries, so the order of the workgroups does not matter; 0: nothing to report):
//   [0] finite      ~0 - k of the first k whose value is NaN / Inf
//   [1] symmetric   partner != NULL (P): ~0 - c, c the smallest min(i, j) over the entries k = (i, j) that differ from src[partner[k]] -- from 0.0 where
//                   partner[k] < 0 -- which is the column layout::csc_asymmetry names.  cp / ri: the pattern as int arrays (the CSR copy of P), ncols columns
//   [2], [3] range  e != NULL: the bits of the largest a = |(T) src[k]| 2^e[k], and ~0 - the bits of the smallest non-zero one (non-negative doubles order as
//                   their bits do): what equil_check_range asks for
// One entry per lane; a wave and then the workgroup reduce first, one atomic per key and workgroup.
constexpr int VALIDATE_VALUES_THREADS = 256;
constexpr int VALIDATE_VERDICT_KEYS = 4;
template <typename T>
void validate_values(hipStream_t st, const double* src, int64_t cnt, const int* partner, const int* cp, const int* ri, int ncols, const int* e,
                     unsigned long long* verdict);
// out[panel][r][16] = sum_k M[r][k] B[panel][k][16] for a plain CSR matrix (k_csr_panel.hip): the check's products of the sparse shared batch.  One 16-lane
// row per (matrix row, panel), spr strips of it for long rows (csr_panel_spr: from the mean row length), fixed summation order, no atomics.
// rowsB / rowsOut: rows per panel of B / out.
template <typename T> struct CsrPanelMatrix { int rows = 0; const int* rp = nullptr; const int* ci = nullptr; const T* va = nullptr; int spr = 1; };
int csr_panel_spr(int64_t nnz, int rows);
template <typename T> void csr_panel(hipStream_t st, const CsrPanelMatrix<T>& M, const T* B, int rowsB, T* out, int rowsOut, int npanel);
template <typename T> void to_panels(hipStream_t st, const double* src, int count, int len, int rowsP, T* dst);     // [count][len] doubles -> panels
template <typename T> void from_panels(hipStream_t st, const T* src, int count, int len, int rowsP, double* dst);   // panels -> [count][len] doubles
template <typename T> void transpose_rowmajor(hipStream_t st, const T* src, int64_t lds, int rows, int cols, T* dst, int64_t ldd);   // dims multiples of 32
// dst[r][c] = scale[r] * src[r][c] for a row-major rows x cols matrix (ld = cols, a multiple of VecOf<T>::N): W = diag(sqrt(s_i)) A of the per-row rho scale
template <typename T> void scale_rows(hipStream_t st, const T* src, const T* scale, int rows, int cols, T* dst);
// w = rho z - y over panels [npanel][MP][16] for the columns of the active mask (rho_row != NULL: rho_i of the row instead of rho): what the rows_zy / rows_zy_scaled
// epilogue leaves behind, re-formed after a switch of the family rho (qps_set_shared_adaptive_rho)
template <typename T> void panel_w(hipStream_t st, const T* z, const T* y, const int* active, const T* rho_row, T rho, int MP, int npanel, T* w);

// ---- polishing step of the shared-matrix batches (k_shared_polish.hip): the kernels of qps_polish.hip on panels, one MINRES per column in lockstep ----------
// A KKT vector is [npanel][rowsN][16] followed by [npanel][rowsM][16] (multiplier block at full length, 0/1 mask).  The products A v_x, P v_x, A'wl with
// wl = mask v_lambda come from the handle's check_products; SharedPolishProducts names their panels.  State: [2][16 npanel], ping-ponged by shared_polish_step.
// live / take: one int per column.  pa / pb: 16 npanel * shared_polish_blocks doubles each (one partial per column and workgroup, added in workgroup order).
struct SharedPolishState { double beta, oldb, dbar, epsln, phibar, cs, sn, bnorm, tol, alfa; int itn, done, flag, maxit; };
struct SharedPolishGeom { int n = 0, m = 0, rowsN = 0, rowsM = 0, npanel = 0; };
template <typename T> struct SharedPolishProducts { const T* mask = nullptr; T* wl = nullptr; const T *Ax = nullptr, *Px = nullptr, *Aty = nullptr; };
int shared_polish_blocks(int rowsN, int rowsM);   // workgroups per panel: from the vector length alone, so a column's sums do not depend on the batch around it
// mask, g = [-q; l or u or 0] and counts[2 b] = numL, counts[2 b + 1] = numU (zero-filled by the caller) from the sign of y       SolveQuadraticProgram.m:293-299
template <typename T>
void shared_polish_setup(hipStream_t st, const SharedPolishGeom& g, const T* q, const T* l, const T* u, const T* y, T* mask, T* gv, int* counts);
template <typename T> void shared_polish_wl(hipStream_t st, const SharedPolishGeom& g, const T* mask, const T* v, T* wl);   // wl = mask v_lambda, every column
// rhs = g - K t on the live columns, from the products of (t_x, wl)
template <typename T>
void shared_polish_rhs(hipStream_t st, const SharedPolishGeom& g, const int* live, const T* gv, const T* t, const SharedPolishProducts<T>& k, T* rhs);
// MINRES start from x0 (products of (x0_x, wl)): r1 = r2 = b - KK x0, w0 = w1 = 0, both halves of `state`; a column that is not live is born done
template <typename T>
void shared_polish_begin(hipStream_t st, const SharedPolishGeom& g, const int* live, T delta, const T* b, const T* x0, const SharedPolishProducts<T>& k, T* r1,
                         T* r2, T* w0, T* w1, double* pa, double* pb, SharedPolishState* state, double tol, int maxit);
// one MINRES iteration of every column that is not done, after the products of (r2_x, wl): c = KK r2, the Lanczos vector over r1 (and wl = mask of it for the
// next product), w over w1, x += phi w, nxt = the next states.  The caller then swaps r1 / r2, w1 / w2 and cur / nxt.
template <typename T>
void shared_polish_step(hipStream_t st, const SharedPolishGeom& g, SharedPolishState* cur, SharedPolishState* nxt, T delta, const SharedPolishProducts<T>& k,
                        T* c, T* r1, T* r2, T* w1, const T* w2, T* x, double* pa, double* pb);
template <typename T> void shared_polish_add(hipStream_t st, const SharedPolishGeom& g, const int* live, const SharedPolishState* state, T* t, T* tt);   // t += tt (:319)
template <typename T> void shared_polish_select(hipStream_t st, const SharedPolishGeom& g, const int* take, const T* t, T* x);   // x = t_x where take (:322-325)
// qps_adjoint_shared, the second caller of the rounds: its set-up (mask and counts from the sign of y as above, g = [g_x; 0]) and its read-out (dq = -t_x,
// dl / du = t_lambda on the rows with y < 0 / y > 0; a column that is not live gives zeros and its t is cleared)
template <typename T> void shared_adjoint_setup(hipStream_t st, const SharedPolishGeom& g, const T* gx, const T* y, T* mask, T* gv, int* counts);
template <typename T> void shared_adjoint_readout(hipStream_t st, const SharedPolishGeom& g, const int* live, const T* y, T* t, T* dq, T* dl, T* du);
// k_value_gradient.hip: out[k] = scale * sum over the 16 npanel columns of  U[a] V[b] + W[b] Z[a]  for the nnz entries k of a CSR pattern, a = rowof[k], b = ci[k];
// U, Z are panels [npanel][rowsA][16], V, W panels [npanel][rowsB][16].  Accumulated in double in a fixed order: independent of the grid, reproducible.
template <typename T>
void panel_value_gradient(hipStream_t st, int64_t nnz, const int* rowof, const int* ci, const T* U, const T* Z, int rowsA, const T* V, const T* W, int rowsB, int npanel,
                          double scale, double* out);

// ---- matrix-free CG of the shared-matrix batches (k_cg_panel.hip): LinOpCg! per column, all columns in lockstep on panels [npanel][n or m][16] ----------------
// State: [2][16 npanel], ping-ponged by cg_panel_iteration (cur -> cur ^ 1); res2 / prev2 are the squared residual norms of cg!.  part_uc holds
// 16 npanel * cg_panel_op_blocks(n, spr_op) doubles, part_rr 16 npanel * cg_panel_vec_blocks(n): one partial per (workgroup, column), added in workgroup order.
struct CgPanelState { double res2, prev2, tol; int itn, done; };
template <typename T> struct CgPanelArgs {
    int n = 0, m = 0, npanel = 0;
    CsrPanelMatrix<T> P, A, At;                  // A.spr: v = rho_i (A u) and the post step; At.spr: the right-hand side
    int spr_op = 1;                              // the strips of "row r of P, then row r of A'": cg_panel_op_spr
    const T *q = nullptr, *lo = nullptr, *hi = nullptr; T *x = nullptr, *xp = nullptr, *z = nullptr, *zp = nullptr, *y = nullptr;   // the ADMM state
    T *xx = nullptr, *r = nullptr, *u = nullptr, *c = nullptr, *v = nullptr, *t = nullptr; const T* w = nullptr;                  // x~, cg!'s vectors, rho_i z - y
    double *part_uc = nullptr, *part_rr = nullptr; CgPanelState* state = nullptr;
    const int* active = nullptr;                 // one word per column
    const T *rho_row = nullptr, *rho1_row = nullptr;   // rho_i and 1 / rho_i per row of A while a scale is set (m long)
    T rho = T(1), sigma = T(0), alpha = T(0);
    // qps_set_shared_column_rho: rho_b and 1 / rho_b per column (16 npanel long) instead of rho; rho_row / rho1_row then hold s_i and 1 / s_i and the kernels
    // multiply.  NULL: the scalar rho, in the instantiations that never read these
    const T *rho_col = nullptr, *rho1_col = nullptr;
    double eps_pcg = 0; int max_it = 0;          // abstol and maxiter of cg!
};
int cg_panel_op_spr(int64_t nnzP, int64_t nnzA, int n);   // from the mean of nnz(row of P) + nnz(row of A'): what one row group of the operator's second launch walks
int cg_panel_op_blocks(int rows, int spr);                // workgroups per panel of the operator's second launch: 16 / spr rows per group, at most 2048 workgroups
int cg_panel_vec_blocks(int rows);                        // workgroups per panel of the vector kernels: 16 rows per group, at most 256 workgroups
// t = sigma x - q + A'w, r = t - Op(x~), u = 0, state[0 .. 16 npanel) with tol = max(sqrt(eps(T)) ||r||, eps_pcg); a column is born done when it is inactive or within tol
template <typename T> void cg_panel_begin(hipStream_t st, const CgPanelArgs<T>& a);
// one iteration of every column that is not done, four launches: fold + u = r + beta u (first: the scalars of `cur` are current), v = rho_i (A u),
// c = P u + sigma u + A'v with the partials of u'c, x~ += alpha u and r -= alpha c with the partials of ||r||^2
template <typename T> void cg_panel_iteration(hipStream_t st, const CgPanelArgs<T>& a, int cur, bool first);
template <typename T> void cg_panel_finish(hipStream_t st, const CgPanelArgs<T>& a, int cur);   // the last ||r||^2 folded into state[cur] in place, before the host reads it
// z~ = A x~ with SolveQuadraticProgram.jl:59-61 as its epilogue, then xp = x, x = alpha x~ + (1 - alpha) x; active columns only
template <typename T> void cg_panel_post(hipStream_t st, const CgPanelArgs<T>& a);
// w = rho_b z - y (rho_b s_i z - y with a row scale) on the active columns: panel_w with the rho of a.rho_col, which must be set
template <typename T> void cg_panel_w(hipStream_t st, const CgPanelArgs<T>& a, T* w);

// ---- small-problem path (k_small.hip): the whole loop in one single-workgroup launch ---------------------------------------
template <typename T> bool admm_small_supported(int n, int m, int NP, int MP);
template <typename T> void transpose_small(hipStream_t st, const T* A, int NP, int MP, T* At);
// batch of small QPs, one workgroup per QP (register-resident kernel): per-QP argument slots are filled on the host with
// admm_small_args_set (an empty iteration window parks a QP), reports come back as admm_small_out_bytes() records
template <typename T> bool admm_small_batch_supported(int NP, int MP);
size_t admm_small_args_bytes();
void admm_small_args_set(void* host_array, int idx, int n, int m, int NP, int MP, int it_begin, int it_end, int numItrConv, int adptRho, double rho,
                         double rhorho, double sigma, double alpha, double epsAbs, double epsRel, double epsAdmm, double fctrRho);
template <typename T>
void admm_small_batch(hipStream_t st, int count, int NP, int MP, const void* args_dev, const T* A, const T* P, const T* S, const T* q, const T* l,
                      const T* u, T* x, T* xp, T* z, T* y, void* outs_dev);
// runs iterations it_begin+1 .. it_end (or until a termination test fires / the proposed rho leaves the fctrRho band);
// out_dev receives {last iteration, convFlag, need_rho, res[8]} (admm_small_out_bytes / admm_small_read)
template <typename T>
void admm_small(hipStream_t st, int n, int m, int NP, int MP, int it_begin, int it_end, int numItrConv, int adptRho, double rho,
                double rhorho, double sigma, double alpha, double epsAbs, double epsRel, double epsAdmm, double fctrRho, const T* A,
                const T* At, const T* P, const T* S, const T* q, const T* l, const T* u, T* x, T* xp, T* z, T* y, void* out_dev);
size_t admm_small_out_bytes();
void admm_small_read(const void* host_copy, int* last_it, int* convFlag, int* need_rho, double* res8);

template <typename T> void fill(hipStream_t st, T* p, int64_t n, T v);
template <typename T> void convert_copy(hipStream_t st, const double* src, T* dst, int64_t n);   // dst[i] = (T)src[i]
template <typename T> void convert_back(hipStream_t st, const T* src, double* dst, int64_t n);   // dst[i] = (double)src[i]
// n host doubles -> device T (or back) through the device staging buffer `stage` (n doubles), then the stream is synchronised: the host array may
// be reused or read at once.  n <= 0 does nothing.
template <typename T> inline hipError_t upload_staged(hipStream_t st, double* stage, const double* h, T* d, int64_t n) {
    if (n <= 0) return hipSuccess;
    const hipError_t e = hipMemcpyAsync(stage, h, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return e;
    convert_copy<T>(st, stage, d, n);
    return hipStreamSynchronize(st);
}
template <typename T> inline hipError_t download_staged(hipStream_t st, double* stage, const T* d, double* h, int64_t n) {
    if (n <= 0) return hipSuccess;
    convert_back<T>(st, d, stage, n);
    const hipError_t e = hipMemcpyAsync(h, stage, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, st);
    return e != hipSuccess ? e : hipStreamSynchronize(st);
}

// ---- setup kernels (k_setup.hip) -----------------------------------------------------------------------------
// dst (row-major rows x NPc, zero padded to rowsP x NPc) = transpose-of-column-major src (rows x cols, ld lds) as T
template <typename T>
void import_colmajor(hipStream_t st, const double* src, int64_t lds, int rows, int cols, T* dst, int64_t ldd);

// C[i][j] (+)= alpha * sum_k opA(i,k) opB(k,j); all dims multiples of 64 (K multiple of 16); row-major C with ldc.
// a_kcontig: opA(i,k) = A[i*lda + k] else A[k*lda + i].  b_kcontig: opB(k,j) = B[j*ldb + k] else B[k*ldb + j].
// lower_only: skip tiles strictly above the block diagonal.  batch: blockIdx.z with element strides sA,sB,sC.
template <typename T>
void gemm(hipStream_t st, int M, int N, int K, T alpha, const T* A, int64_t lda, bool a_kcontig, const T* B, int64_t ldb,
          bool b_kcontig, T beta, T* C, int64_t ldc, bool lower_only, int batch = 1, int64_t sA = 0, int64_t sB = 0,
          int64_t sC = 0, int ktri = 0);
// ktri: 1 = opB lower triangular (k loop starts at the tile's first column), 2 = opA lower triangular (k loop stops
// after the tile's last row), 3 = opA upper triangular, 4 = opB upper triangular (k loop stops after the tile's last column): structurally zero
// k-tiles are skipped.

// M = PI + rho * AA (lower triangle incl. diagonal tiles; NP x NP)   (LinearSystemSolvers.jl:114,128)
template <typename T> void assemble_M(hipStream_t st, int NP, const T* PI, const T* AA, T rho, T* M, int batch = 1,
                                      const double* rho_arr = nullptr);   // rho_arr: per-QP rho (device) for a batch
// PI = P + sigma I on the n x n part, identity on the padding diagonal (keeps the padded factor well defined)
template <typename T> void make_PI(hipStream_t st, int n, int NP, const T* P, T sigma, T* PI, int batch = 1);

// Blocked right-looking Cholesky of the NP x NP row-major matrix M (lower), in place.  dinv receives the inverses of
// the 64 x 64 diagonal blocks (NP/64 blocks of 64*64).  fail_dev: int32, 0 or 1+index of the failing pivot.
// scratch != nullptr: chol_scratch_elems(NP) elements per matrix (consecutive); selects the 128-column steps (one panel launch + one
// GEMM launch per 128 columns).  Any buffer that is dead during the factorisation will do (the sweep matrix S, for instance).
inline int64_t chol_scratch_elems(int NP) { return (int64_t)((NP / 64 + 1) / 2) * 3 * 4096 + 64; }   // stash tiles + the hand-off counter of k_chol_update_diag
inline bool chol_scratch_fits(int NP) { return chol_scratch_elems(NP) <= (int64_t)NP * NP; }   // an NP x NP buffer is large enough (NP >= 128)
template <typename T> void cholesky(hipStream_t st, int NP, T* M, T* dinv, int* fail_dev, int batch = 1, T* scratch = nullptr);   // batch: matrices NP*NP apart

// Build the sweep matrix S from L (lower of M) and the 64-block inverses: diagonal nb-blocks inverted by recursive
// doubling, then mirrored into the upper triangle.  tmp: NP x NP scratch.
// premul (single matrix, nb < NP): every block row is additionally multiplied by its inverted diagonal block and negated off the diagonal
// (lower blocks -W_JJ L_JK, upper blocks -(L_KJ W_JJ)'): the form the single-launch blocked sweeps read (k_trsv_blocked.hip).
template <typename T> void build_sweep_matrix(hipStream_t st, int NP, int nb, const T* L, const T* dinv, T* S, T* tmp, int batch = 1, bool premul = false);

// ---- blocked triangular substitution, one launch per sweep (k_trsv_blocked.hip) ----------------------------------------------------
// out = forward (bwd = false: rows of S left of and inside the diagonal block) or backward (bwd = true) sweep over the PREMULTIPLIED sweep
// matrix with nb x nb blocks.  pub: trsv_blocked_pub_words<T>(NP) 64-bit words, zero-filled once (hand-off granules); epoch: a value that grows
// with every launch on this pub buffer (never 0); abort_word: set to 1 by a launch that gave up waiting (its `out` is garbage then).
template <typename T> bool trsv_blocked_supported(int NP, int nb);   // on the CURRENT device (co-residency of the 256 workgroups checked per device)
template <typename T> int64_t trsv_blocked_pub_words(int NP);
// Scope around the launches of one forward + backward pair: chains the pair behind the previous blocked-sweep launches of the device
// when those went to another stream, so that two of these persistent launches never share the chip (k_trsv_blocked.hip, "Co-residency").
struct TrsvBlockedPair { int dev; hipStream_t stream; TrsvBlockedPair(int device, hipStream_t st); ~TrsvBlockedPair(); TrsvBlockedPair(const TrsvBlockedPair&) = delete; };
void trsv_blocked_forget_stream(int device, hipStream_t st);   // a handle's stream is about to be recycled / destroyed (it is idle)
template <typename T>
void trsv_blocked(hipStream_t st, bool bwd, const T* S, int64_t ld, int NP, int nb, const T* v, T* out, unsigned long long* pub,
                  unsigned epoch, unsigned* abort_word, int mode = 0);

}  // namespace qps
