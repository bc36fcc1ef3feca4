// k_pass_w.hip -- the two-launch iteration of a dense fp64 handle that solves on its cached factor, in whitened coordinates.
//
// With M = P + sigma I + rho A'A = L L', W = inv(L):  B = A W' (m x n), G = W W' (symmetric), c = W q; the iterate is carried as u = W t and p = W x.
// One reference iteration (SolveQuadraticProgram.jl:54-61, LinearSystemSolvers.jl:134-139) is then
//     z~ = B u,  z / y row updates as they are,  w = rho z - y,  e = B'w
//     p+ = alpha G u + (1 - alpha) p            (:57 multiplied by W)
//     u+ = sigma p+ - c + e                     (LinearSystemSolvers.jl:136 multiplied by W)
// G u depends on u alone, so nothing has to finish between the sweep and the pass: k_wpass streams the stacked matrix [B ; lower triangle of G] in ONE
// launch (the row tile of the fused A-pass, k_pass_kernel.h: row dot, row statement by the owner thread, column accumulation of the same registers) and
// k_wsum adds the slabs in fixed order and forms p+ and u+.  The check reads neither A nor B again: a = A x is carried by its own recurrence in the row
// owners, B'y is a third accumulator, and x, x - xp, A'y come from one pass over the triangle of L for three right-hand sides (k_lpass3).
#include "k_pass_kernel.h"

namespace qps {

namespace {

constexpr int WPASS_WGS = 256;   // one workgroup per CU; also the slab count of every slab set

template <typename T, int THREADS, int KC, int R, bool CHECK>
__global__ __launch_bounds__(THREADS) void k_wpass(WhitenedPass<T> a) {
    using PS = Pass<T, THREADS, KC, R, CHECK>;
    using V = typename PS::V;
    constexpr int VN = PS::VN, CHUNK = PS::CHUNK, WAVES = PS::WAVES;
    const int tid = threadIdx.x, g = blockIdx.x, G = gridDim.x;
    const int NP = a.NP, MP = a.MP;
    const int64_t ld = a.ld;
    const T alpha = a.alpha, rho = a.rho;
    const T alpha1 = T(1) - alpha, rho1 = T(1) / rho;
    // rows of B of this workgroup (none: it only takes triangle tiles and leaves a zero slab of B'w)
    const int row0 = min(MP, g * a.rows_per_wg), row1 = min(MP, row0 + a.rows_per_wg);
    const int nB = (row1 - row0) / R;                     // rows_per_wg and MP are multiples of 4 >= R
    // triangle tiles of R rows, longest first, dealt in alternating direction over the workgroups so that every pair of rounds carries the same bytes
    const int ntiles = NP / R, full = ntiles / G, rem = ntiles - full * G;
    auto slot_of = [&](int it) { return it * G + ((it & 1) ? G - 1 - g : g); };
    const int nT = full + (slot_of(full) - full * G < rem ? 1 : 0);
    const int nt = nB + nT;
    auto is_tri = [&](int t) { return t >= nB; };         // after its rows of B a workgroup takes its triangle tiles (triangle first: 61 -> 63 us on C2)
    auto tile_row = [&](int t) { return t < nB ? row0 + t * R : (ntiles - 1 - slot_of(t - nB)) * R; };

    __shared__ T red[2][WAVES][R];
    __shared__ T wsh[2][R];
    __shared__ T ysh[2][R];

    V xv[KC];   // this thread's slice of u
#pragma unroll
    for (int k = 0; k < KC; ++k) {
        const int c = tid * VN + k * CHUNK;
        if (c < NP) xv[k] = *reinterpret_cast<const V*>(a.u + c);
        else { T* p = reinterpret_cast<T*>(&xv[k]);
#pragma unroll
            for (int e = 0; e < VN; ++e) p[e] = T(0); }
    }
    T acc[KC][VN], acc2[KC][VN], acc3[KC][VN];
#pragma unroll
    for (int k = 0; k < KC; ++k)
#pragma unroll
        for (int e = 0; e < VN; ++e) { acc[k][e] = T(0); acc2[k][e] = T(0); acc3[k][e] = T(0); }
    unsigned long long m_res = 0ull, m_ax = 0ull, m_z = 0ull, m_dz = 0ull;   // owned by threads tid < R

    // per-row scalars of a tile, prefetched by the R owner threads: z, y, l, u, a of a row of B; u_r and G_rr of a triangle row
    auto load = [&](V (&b)[R][KC], int t, T& o0, T& o1, T& o2, T& o3, T& o4) {
        const int row = tile_row(t);
        if (!is_tri(t)) {
            PS::load_tile(b, a.B, ld, row, NP, tid);
            if (tid < R) { o0 = a.z[row + tid]; o1 = a.y[row + tid]; o2 = a.l[row + tid]; o3 = a.hi[row + tid]; o4 = a.a[row + tid]; }
        } else {
#pragma unroll
            for (int i = 0; i < R; ++i)
#pragma unroll
                for (int k = 0; k < KC; ++k) {
                    const int c = tid * VN + k * CHUNK;
                    T* p = reinterpret_cast<T*>(&b[i][k]);
                    if (c <= row + i) {   // (row + i < NP: the vector lies inside the row)
                        // Plain loads, unlike B's: the triangle (67 MB on C2) is read again by the next launch and fits the Infinity Cache beside the
                        // non-temporal stream of B (measured on C2: 60.0 -> 56.9 us per launch; non-temporal and clamped 62.4, plain and clamped 58.8)
                        typedef T NV __attribute__((ext_vector_type(VN)));
                        const NV v = *reinterpret_cast<const NV*>(a.G + (int64_t)(row + i) * ld + c);
#pragma unroll
                        for (int e = 0; e < VN; ++e) p[e] = v[e];
                    } else {
#pragma unroll
                        for (int e = 0; e < VN; ++e) p[e] = T(0);
                    }
                }
            if (tid < R) { o0 = a.u[row + tid]; o1 = a.G[(int64_t)(row + tid) * (ld + 1)]; }
        }
    };
    auto process = [&](V (&b)[R][KC], int t, T o0, T o1, T o2, T o3, T o4, int par) {
        const int row = tile_row(t);
        const bool tri = is_tri(t);                        // workgroup-uniform
        if (tri) {
            // strictly lower entries only: the diagonal is counted once, by the row owner
#pragma unroll
            for (int i = 0; i < R; ++i)
#pragma unroll
                for (int k = 0; k < KC; ++k) {
                    T* ap = reinterpret_cast<T*>(&b[i][k]);
#pragma unroll
                    for (int e = 0; e < VN; ++e) if (tid * VN + k * CHUNK + e >= row + i) ap[e] = T(0);
                }
            if (tid < R) wsh[par][tid] = o0;             // u_r, known before the dot: a triangle tile needs one barrier only
        }
        T d[R];
#pragma unroll
        for (int i = 0; i < R; ++i) {
            T s = T(0);
#pragma unroll
            for (int k = 0; k < KC; ++k) {
                const T* ap = reinterpret_cast<const T*>(&b[i][k]);
                const T* xp_ = reinterpret_cast<const T*>(&xv[k]);
#pragma unroll
                for (int e = 0; e < VN; ++e) s += ap[e] * xp_[e];
            }
            d[i] = wave_sum_all(s);
        }
        if ((tid & 63) == 0) {
#pragma unroll
            for (int i = 0; i < R; ++i) red[par][tid >> 6][i] = d[i];
        }
        __syncthreads();
        if (tid < R) {
            T zt = T(0);
#pragma unroll
            for (int w = 0; w < WAVES; ++w) zt += red[par][w][tid];   // fixed order
            if (tri) {
                a.gd[row + tid] = zt + o1 * o0;        // d_r = sum_{c <= r} G[r][c] u[c]
            } else {
                const T zo = o0, yo = o1, lo = o2, hi = o3;
                T zn, yn;
                const T t = alpha * zt + alpha1 * zo + rho1 * yo;                  // :60
                zn = t > hi ? hi : (t < lo ? lo : t);                               //     clamp(., vL, vU)
                yn = yo + rho * (alpha * zt + alpha1 * zo - zn);                    // :61
                wsh[par][tid] = rho * zn - yn;                                      // LinearSystemSolvers.jl:134
                a.z[row + tid] = zn;
                a.y[row + tid] = yn;
                const T ax = alpha * zt + alpha1 * o4;                            // A x+ = alpha A x~ + (1 - alpha) A x   (:57 multiplied by A)
                a.a[row + tid] = ax;
                if (CHECK) {
                    ysh[par][tid] = yn;
                    m_res = umax(m_res, absbits((double)(ax - zn)));                // :85
                    m_ax = umax(m_ax, absbits((double)ax));                         // :88
                    m_z = umax(m_z, absbits((double)zn));
                    m_dz = umax(m_dz, absbits((double)(zn - zo)));                  // :105
                }
            }
        }
        if (tri) {
#pragma unroll
            for (int i = 0; i < R; ++i) {
                const T w = wsh[par][i];
#pragma unroll
                for (int k = 0; k < KC; ++k) {
                    const T* ap = reinterpret_cast<const T*>(&b[i][k]);
#pragma unroll
                    for (int e = 0; e < VN; ++e) acc2[k][e] += ap[e] * w;
                }
            }
            // (keeps this tail distinct from the one below: merged, the two accumulators are reached through a selected pointer and live in scratch)
            asm volatile("");
        } else {
            __syncthreads();
#pragma unroll
            for (int i = 0; i < R; ++i) {
                const T w = wsh[par][i];
                const T yw = CHECK ? ysh[par][i] : T(0);
#pragma unroll
                for (int k = 0; k < KC; ++k) {
                    const T* ap = reinterpret_cast<const T*>(&b[i][k]);
#pragma unroll
                    for (int e = 0; e < VN; ++e) { acc[k][e] += ap[e] * w; if constexpr (CHECK) acc3[k][e] += ap[e] * yw; }
                }
            }
        }
    };

    // LDS of parity `par` is written again two tiles later, behind the first barrier of the tile in between: every reader of this tile has passed it
    V bufA[R][KC], bufB[R][KC];
    T a0 = T(0), a1 = T(0), a2 = T(0), a3 = T(0), a4 = T(0), b0 = T(0), b1 = T(0), b2 = T(0), b3 = T(0), b4 = T(0);
    if (nt > 0) load(bufA, 0, a0, a1, a2, a3, a4);
    for (int t = 0; t < nt; t += 2) {
        const bool haveB = t + 1 < nt;
        if (haveB) load(bufB, t + 1, b0, b1, b2, b3, b4);
        process(bufA, t, a0, a1, a2, a3, a4, 0);
        if (haveB) {
            if (t + 2 < nt) load(bufA, t + 2, a0, a1, a2, a3, a4);
            process(bufB, t + 1, b0, b1, b2, b3, b4, 1);
        }
    }

    // slabs of column sums (zeros where a workgroup had no rows of that kind, so k_wsum adds every slab unconditionally); write-through stores
#pragma unroll
    for (int k = 0; k < KC; ++k) {
        const int c = tid * VN + k * CHUNK;
        if (c < NP) {
            typedef T NVS __attribute__((ext_vector_type(VN)));
            NVS o1, o2;
#pragma unroll
            for (int e = 0; e < VN; ++e) { o1[e] = acc[k][e]; o2[e] = acc2[k][e]; }
            __builtin_nontemporal_store(o1, reinterpret_cast<NVS*>(a.slab_e + (int64_t)g * a.part_ld + c));
            __builtin_nontemporal_store(o2, reinterpret_cast<NVS*>(a.slab_g + (int64_t)g * a.part_ld + c));
            if constexpr (CHECK) {
                NVS o3;
#pragma unroll
                for (int e = 0; e < VN; ++e) o3[e] = acc3[k][e];
                __builtin_nontemporal_store(o3, reinterpret_cast<NVS*>(a.slab_y + (int64_t)g * a.part_ld + c));
            }
        }
    }
    if (CHECK && tid < R) {
        if (m_res) atomicMax(&a.slots[0], m_res);
        if (m_ax) atomicMax(&a.slots[2], m_ax);
        if (m_z) atomicMax(&a.slots[3], m_z);
        if (m_dz) atomicMax(&a.slots[8], m_dz);
    }
}

// One launch, fixed order: per column the sums of NS slab sets (k_colsum's walk: a workgroup owns one 128-byte line of every slab row), then
//     g = gd + sum slabs_g,  p+ = alpha g + (1 - alpha) p,  u+ = sigma p+ - c + sum slabs_e,  (NS == 3) bty = sum slabs_y.
// first: no pass has run yet (z = y = 0, no slabs): p+ = p, u+ = sigma p - c.
template <typename T, int NS>
__global__ __launch_bounds__(256) void k_wsum(WhitenedSum<T> a) {
    using V = typename VecOf<T>::type;
    constexpr int VN = VecOf<T>::N;
    constexpr int COLS = 128 / (int)sizeof(T), CL = COLS / VN, TL = 256 / CL, PL = 256 / COLS;
    static_assert(PL == 16 && TL % PL == 0, "fp64 geometry of k_colsum");
    const int cl = threadIdx.x % CL, tl = threadIdx.x / CL;
    const int c = blockIdx.x * COLS + cl * VN;
    const int ntiles = a.first ? 0 : a.ntiles;
    const T* sets[3] = {a.slab_e, a.slab_g, a.slab_y};
    __shared__ T red[NS][TL][COLS + 1];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        T acc[VN];
#pragma unroll
        for (int e = 0; e < VN; ++e) acc[e] = T(0);
        if (c < a.ncols) {
            int t = tl;
            for (; t + 7 * TL < ntiles; t += 8 * TL) {
                V v[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = *reinterpret_cast<const V*>(sets[s] + (int64_t)(t + TL * j) * a.part_ld + c);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const T* vp = reinterpret_cast<const T*>(&v[j]);
#pragma unroll
                    for (int e = 0; e < VN; ++e) acc[e] += vp[e];
                }
            }
            for (; t < ntiles; t += TL) {
                const V v = *reinterpret_cast<const V*>(sets[s] + (int64_t)t * a.part_ld + c);
                const T* vp = reinterpret_cast<const T*>(&v);
#pragma unroll
                for (int e = 0; e < VN; ++e) acc[e] += vp[e];
            }
        }
#pragma unroll
        for (int e = 0; e < VN; ++e) red[s][tl][cl * VN + e] = acc[e];
    }
    __syncthreads();
    const int o = threadIdx.x / PL, pl = threadIdx.x % PL;
    T sum[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        T v = T(0);
#pragma unroll
        for (int k = 0; k < TL / PL; ++k) v += red[s][pl * (TL / PL) + k][o];
        sum[s] = row16_sum_last(v);
    }
    const int oc = blockIdx.x * COLS + o;
    if (pl == PL - 1 && oc < a.ncols) {
        T pn = a.p_old[oc];
        if (!a.first) { const T gv = a.gd[oc] + sum[1]; pn = a.alpha * gv + (T(1) - a.alpha) * pn; }
        a.p_new[oc] = pn;
        a.u[oc] = a.sigma * pn - a.c[oc] + sum[0];
        if (NS == 3) a.bty[oc] = sum[2];
    }
}

// x = L p+,  max |L (p+ - p)|  (slot 7: norm(vX - vXP, Inf), SolveQuadraticProgram.jl:105),  aty = L bty: the lower triangle of L is read once for the three
// right-hand sides.  RB rows per workgroup, long rows first, as k_gemv_rows with TRI = 1.
template <typename T, int RB, int THREADS>
__global__ __launch_bounds__(THREADS) void k_lpass3(const T* __restrict__ L, int64_t ld, const T* __restrict__ pn, const T* __restrict__ po,
                                                    const T* __restrict__ bty, T* __restrict__ x, T* __restrict__ aty,
                                                    unsigned long long* __restrict__ slots) {
    using V = typename VecOf<T>::type;
    constexpr int VN = VecOf<T>::N, CHUNK = THREADS * VN, WAVES = THREADS / 64;
    const int tid = threadIdx.x;
    const int rb = (int)(gridDim.x - 1 - blockIdx.x) * RB;
    const int ce = rb + RB;                                // (RB is a multiple of VN: whole vectors)
    T acc[3][RB];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int i = 0; i < RB; ++i) acc[j][i] = T(0);
    const T* Lrow = L + (int64_t)rb * ld;
#pragma unroll 4
    for (int c = tid * VN; c < ce; c += CHUNK) {
        const V v0 = *reinterpret_cast<const V*>(pn + c), vo = *reinterpret_cast<const V*>(po + c), v2 = *reinterpret_cast<const V*>(bty + c);
        const T *p0 = reinterpret_cast<const T*>(&v0), *pp = reinterpret_cast<const T*>(&vo), *p2 = reinterpret_cast<const T*>(&v2);
#pragma unroll
        for (int i = 0; i < RB; ++i) {
            const V lv = *reinterpret_cast<const V*>(Lrow + (int64_t)i * ld + c);
            const T* lp = reinterpret_cast<const T*>(&lv);
#pragma unroll
            for (int e = 0; e < VN; ++e) {
                const T le = (c + e) <= (rb + i) ? lp[e] : T(0);
                acc[0][i] += le * p0[e];
                acc[1][i] += le * (p0[e] - pp[e]);
                acc[2][i] += le * p2[e];
            }
        }
    }
    __shared__ T red[WAVES][3 * RB];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int i = 0; i < RB; ++i) acc[j][i] = wave_sum_all(acc[j][i]);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int i = 0; i < RB; ++i) red[tid >> 6][j * RB + i] = acc[j][i];
    }
    __syncthreads();
    if (tid < 3 * RB) {
        T s = T(0);
#pragma unroll
        for (int w = 0; w < WAVES; ++w) s += red[w][tid];   // fixed order
        const int j = tid / RB, r = rb + tid % RB;
        if (j == 0) x[r] = s;
        else if (j == 2) aty[r] = s;
        else { const unsigned long long k = absbits((double)s); if (k) atomicMax(&slots[7], k); }
    }
}

template <typename T> __global__ void k_tril_copy(const T* __restrict__ S, T* __restrict__ D, int NP) {
    const int r = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
    if (c < NP) D[(int64_t)r * NP + c] = c <= r ? S[(int64_t)r * NP + c] : T(0);
}

template <typename K, typename A> void launch_timed(K kernel, dim3 grid, dim3 block, hipStream_t st, const A& args) {
    if (g_launch_timing.start) {   // profiled launch: the dispatch's own timestamps (qps_kernels.h)
        const LaunchTiming lt = g_launch_timing;
        g_launch_timing = LaunchTiming();
        hipExtLaunchKernelGGL(kernel, grid, block, 0, st, lt.start, lt.stop, 0, args);
        return;
    }
    hipLaunchKernelGGL(kernel, grid, block, 0, st, args);
}

}  // namespace

bool whitened_supported(int NP, int MP) { return MP > 0 && NP <= 8 * 512 * VecOf<double>::N; }   // the 512-thread instantiations of the pass
int whitened_slabs() { return WPASS_WGS; }

void whitened_pass(hipStream_t st, bool check, WhitenedPass<double> a) {
    using T = double;
    // the launch always has WPASS_WGS workgroups: the rows of B are split over exactly those, in multiples of the largest row tile
    // (apass_plan's split follows QPS_PASS_WGS, which sizes the classic pass's launch and not this one)
    a.rows_per_wg = (((a.MP + WPASS_WGS - 1) / WPASS_WGS + 3) / 4) * 4;
    const int kc = (a.NP + 512 * VecOf<T>::N - 1) / (512 * VecOf<T>::N);
#define QPS_WPASS(KC, R, RC)                                                                                          \
    do {                                                                                                              \
        if (check) launch_timed(k_wpass<T, 512, KC, RC, true>, dim3(WPASS_WGS), dim3(512), st, a);                    \
        else launch_timed(k_wpass<T, 512, KC, R, false>, dim3(WPASS_WGS), dim3(512), st, a);                          \
    } while (0)
    // (row tile of the plain variant, row tile of the check variant): sized so that neither spills
    if (kc <= 1) QPS_WPASS(1, 4, 4);
    else if (kc <= 2) QPS_WPASS(2, 4, 4);
    else if (kc <= 4) QPS_WPASS(4, 4, 2);
    else QPS_WPASS(8, 1, 1);
#undef QPS_WPASS
}

void whitened_sum(hipStream_t st, bool with_bty, const WhitenedSum<double>& a) {
    const dim3 grid((a.ncols + 15) / 16);
    if (with_bty) launch_timed(k_wsum<double, 3>, grid, dim3(256), st, a);
    else launch_timed(k_wsum<double, 2>, grid, dim3(256), st, a);
}

void whitened_lpass(hipStream_t st, const double* L, int64_t ld, int NP, const double* pn, const double* po, const double* bty, double* x, double* aty,
                    unsigned long long* slots) {
    hipLaunchKernelGGL((k_lpass3<double, 4, 512>), dim3(NP / 4), dim3(512), 0, st, L, ld, pn, po, bty, x, aty, slots);
}

void tril_copy(hipStream_t st, const double* S, double* D, int NP) {
    hipLaunchKernelGGL((k_tril_copy<double>), dim3((NP + 255) / 256, NP), dim3(256), 0, st, S, D, NP);
}

}  // namespace qps
