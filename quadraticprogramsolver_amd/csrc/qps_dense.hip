// qps_dense.hip -- DenseSolver: the device-resident ADMM loop driver of a dense handle (Cholesky path) and its plugin calls, behind make_dense (qps_internal.h).
//
// Loop structure follows SolveQuadraticProgram.jl:36-73; the linear solve is the reduced form of
// LinearSystemSolvers.jl:110-142 with cg! replaced by Cholesky + two triangular sweeps (ProxQP.jl:175-206,221-225).
#include <memory>
#include <type_traits>

#include "admm_loop.h"
#include "dense_chol.h"
#include "dense_whitened.h"
#include "qps_batch.h"
#include "qps_internal.h"
#include "qps_kernels.h"
#include "qps_polish.h"

namespace qps {
namespace {

// =================================================================================================================
// Dense problem, Cholesky path
// =================================================================================================================
template <typename T> struct DenseSolver : SolverBase {
    int NP = 0, MP = 0;
    T *A = nullptr, *P = nullptr, *q = nullptr, *l = nullptr, *u = nullptr;
    T *PI = nullptr, *AA = nullptr, *M = nullptr, *S = nullptr, *tmp = nullptr, *dinv = nullptr; int* fail = nullptr;
    T *x = nullptr, *xp = nullptr, *z = nullptr, *zp = nullptr, *y = nullptr, *xx = nullptr, *zz = nullptr, *tt = nullptr, *yv = nullptr;
    T *part = nullptr, *part2 = nullptr, *sw_part = nullptr, *Ax = nullptr, *Px = nullptr, *Aty = nullptr;
    T* At = nullptr; void* small_out = nullptr; void* small_out_host = nullptr; bool small_ok = false;   // small-problem path
    StreamLease lease; Arena arena;   // destroyed in reverse: the device block first, then the stream lease, then the base's Profiler
    double* stage_mat = nullptr; int64_t stage_mat_count = 0;
    int pass_slabs = 0, pass_rpw = 0;   // fused-pass plan (0 slabs: shape not supported, unfused loop only)
    unsigned long long* scratch = nullptr; double* res_dev = nullptr; double* res_host = nullptr; double* stage = nullptr;
    bool have_AA = false, factor_valid = false; double fac_rho = 0, fac_sigma = 0; int fac_nb = 0;
    int nb = 2048; int part_tiles = 0; int num_factorizations = 0;
    // single-launch blocked sweeps (k_trsv_blocked.hip): hand-off granules, launch epoch, give-up word; `blocked_off` while the solve whose
    // launch gave up is being repeated on the multi-launch substitution (the next solve tries the blocked sweeps again)
    unsigned long long* pub = nullptr; unsigned* abort_dev = nullptr; unsigned sweep_epoch = 0; bool blocked_off = false, fac_premul = false;
    bool use_blocked() const { return !blocked_off && trsv_blocked_supported<T>(NP, nb); }
    // hipGraph replay of runs of plain iterations (no check, no rho switch) for problems small enough to be launch bound
    struct IterGraph { int count; const void* xa; double rho, sigma, alpha; int nb; hipGraphExec_t exec; };
    std::vector<IterGraph> graphs;
    bool graphs_disabled = false;
    void drop_graphs() { for (auto& gr : graphs) (void)hipGraphExecDestroy(gr.exec); graphs.clear(); }
    // `count` (even) plain iterations of the fused loop starting with x in `xa`, xp in `xb`; captured once per (count, roles, scalars)
    hipGraphExec_t iter_graph(int count, T* xa, T* xb, double rho, double sigma, double alpha) {
        for (auto& gr : graphs) if (gr.count == count && gr.xa == xa && gr.rho == rho && gr.sigma == sigma && gr.alpha == alpha && gr.nb == nb) return gr.exec;
        if (graphs_disabled) return nullptr;
        if (graphs.size() >= 8) drop_graphs();
        hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr;
        if (hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) != hipSuccess) { (void)hipGetLastError(); graphs_disabled = true; return nullptr; }
        for (int k = 0; k < count; ++k) {
            colsum<T>(st, part, NP, pass_slabs, xa, (T)sigma, q, T(-1), tt, NP);                    // LinearSystemSolvers.jl:136
            sweeps();                                                                               // :137 (profiling is off here: plain launches)
            apass<T>(st, false, A, NP, NP, MP, xx, xa, xb, z, y, l, u, (T)alpha, (T)rho, part, part2, NP, scratch);   // :56-61, :139, next :134-135
            std::swap(xa, xb);
        }
        // nothing was enqueued while capturing, so a failure here just means: run this handle's iterations eagerly from now on
        if (hipStreamEndCapture(st, &graph) != hipSuccess || graph == nullptr) { (void)hipGetLastError(); graphs_disabled = true; return nullptr; }
        const hipError_t e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        if (e != hipSuccess) { (void)hipGetLastError(); graphs_disabled = true; return nullptr; }
        graphs.push_back({count, xa, rho, sigma, alpha, nb, exec});   // (xa is back in its original role: count is even)
        return exec;
    }
    int prof_iter = 0;   // iteration index seen by the level-1 sampler (one bracketed launch per kernel kind per 50 iterations)
    int sample_lvl(int slot) const { return (prof.level == 1 && prof_iter % 50 == slot) ? 1 : 2; }
    int cat_atw, cat_colsum, cat_fwd, cat_bwd, cat_ax, cat_upd, cat_chk, cat_pass, cat_passchk, cat_sweep, cat_xsum, cat_small;
    // Whitened two-launch iteration of solves on the cached factor (fp64 only; dense_whitened.h).  Declared after `arena`: its block is freed before the lease goes.
    std::conditional_t<std::is_same<T, double>::value, WhitenedState, NoWhitenedState> wh;
    WhitenedView<T> whitened_view() const { return {st, NP, MP, A, S, tmp}; }

    DenseSolver(int dev, int64_t n_, int64_t m_, int dt) {
        device = dev; n = n_; m = m_; dtype = dt;
        HIPC(hipSetDevice(device));
        NP = roundup(n, 64); MP = roundup(m, 64);
        const int64_t nn = (int64_t)NP * NP;
        part_tiles = gemv_cols_tiles(MP);
        pass_slabs = apass_plan<T>(NP, MP, &pass_rpw);
        const int slabs = std::max(std::max(part_tiles, pass_slabs), 1);
        small_ok = admm_small_supported<T>((int)n, (int)m, NP, MP);
        // staging area of the matrix import (column-major doubles): inside the arena when the matrices are small
        stage_mat_count = std::max((int64_t)n * n, (int64_t)m * n);
        if (stage_mat_count > ((int64_t)1 << 20)) stage_mat_count = 0;
        auto layout = [&](Arena& ar) {
            A = ar.take<T>((int64_t)MP * NP); P = ar.take<T>(nn); q = ar.take<T>(NP); l = ar.take<T>(MP); u = ar.take<T>(MP);
            PI = ar.take<T>(nn); AA = ar.take<T>(nn); M = ar.take<T>(nn); S = ar.take<T>(nn); tmp = ar.take<T>(nn);
            dinv = ar.take<T>((int64_t)(NP / 64) * 4096); fail = ar.take<int>(4);
            x = ar.take<T>(NP); xp = ar.take<T>(NP); xx = ar.take<T>(NP); tt = ar.take<T>(NP); yv = ar.take<T>(NP);
            z = ar.take<T>(MP); zp = ar.take<T>(MP); y = ar.take<T>(MP); zz = ar.take<T>(MP);
            part = ar.take<T>((int64_t)slabs * NP);
            part2 = ar.take<T>((int64_t)slabs * NP);
            sw_part = ar.take<T>((int64_t)std::max(sweep_fused_slabs<T>(NP), 1) * NP);
            Ax = ar.take<T>(MP); Px = ar.take<T>(NP); Aty = ar.take<T>(NP);
            scratch = ar.take<unsigned long long>(16); res_dev = ar.take<double>(16);
            pub = ar.take<unsigned long long>(trsv_blocked_pub_words<T>(NP));
            abort_dev = reinterpret_cast<unsigned*>(res_dev + 14);   // rides in the check's read-back (slots 8..15 are unused by the check kernels)
            stage = ar.take<double>((int64_t)NP + 2 * (int64_t)MP + 64);
            if (small_ok) { At = ar.take<T>((int64_t)NP * MP); small_out = ar.take<double>(32); }
            if (stage_mat_count > 0) stage_mat = ar.take<double>(stage_mat_count);
        };
        layout(arena);
        st = prof.st = lease.acquire(device, arena.planned());                // stream, pinned block and maybe a recycled device block
        HandleResources& res = lease.res;
        char* const recycled = res.block; res.block = nullptr;                // owned by the arena from here on
        arena.commit(st, recycled, res.block_bytes);
        layout(arena);
        res_host = reinterpret_cast<double*>(res.pinned);                     // one pinned block: check results | small-kernel report
        small_out_host = small_ok ? reinterpret_cast<char*>(res.pinned) + 16 * sizeof(double) : nullptr;
        const double s = sizeof(T);
        // algorithmic bytes per launch (SURVEY §8d "per-kernel algorithmic bytes")
        cat_atw = prof.category("gemv_cols(A'w)", s * ((double)m * n + m + n));
        cat_colsum = prof.category("colsum(rhs)", s * ((double)part_tiles * n + 3.0 * n));
        cat_fwd = prof.category("trsv_forward", s * ((double)n * (n + 1) / 2 + 2.0 * n));
        cat_bwd = prof.category("trsv_backward", s * ((double)n * (n + 1) / 2 + 2.0 * n));
        cat_ax = prof.category("gemv_rows(Ax~)", s * ((double)m * n + m + n));
        cat_upd = prof.category("admm_update", s * (3.0 * n + 7.0 * m));
        cat_chk = prof.category("check_convergence", s * (2.0 * m * n + (double)n * n + 4.0 * n + 4.0 * m));
        // fused pass: A once + x~, x, z, y, l, u in, x, z, y out (s*m*n + vector traffic)
        cat_pass = prof.category("apass(fused A-pass)", s * ((double)m * n + 3.0 * n + 6.0 * m));
        cat_passchk = prof.category("apass(check variant)", s * ((double)m * n + 4.0 * n + 6.0 * m));
        // fused forward+backward sweep: the bytes this kernel has to move -- the triangle ONCE (n(n+1)/2) plus its slabs; SURVEY §8d's
        // figure for the two separate sweeps it replaces is twice the triangle (bench.py reports that one as `two_sweep_algo_GBs`)
        cat_sweep = prof.category("sweeps(fused fwd+bwd, triangle read once)", s * ((double)n * (n + 1) / 2 + 2.0 * n + (double)sweep_fused_slabs<T>(NP) * n));
        cat_xsum = prof.category("colsum(x~ slabs)", s * ((double)sweep_fused_slabs<T>(NP) * n + n));
        wh.categories(prof, (double)n, (double)m);
        // single-launch small-problem loop: bytes PER ITERATION (one launch runs many; bench.py multiplies by the iterations it timed)
        cat_small = prof.category("admm_small(whole loop in one launch; bytes per iteration)", s * ((double)m * n + (double)n * n) + s * (6.0 * n + 10.0 * m));
    }
    ~DenseSolver() override {
        (void)hipSetDevice(device);
        (void)hipStreamSynchronize(st);
        trsv_blocked_forget_stream(device, st);   // the stream goes back to the pool (or is destroyed): the sweep gate must not record on it
        drop_graphs();
        prof.release_events();
        lease.res.block = arena.base; lease.res.block_bytes = arena.bytes; arena.base = nullptr;   // the block goes back with the lease
    }

    // host double array -> device T vector (zero padded allocation is preserved beyond `count`)
    void upload_vec(const double* h, T* d, int64_t count) { HIPC(upload_staged<T>(st, stage, h, d, count)); }
    void download_vec(const T* d, double* h, int64_t count) { HIPC(download_staged<T>(st, stage, d, h, count)); }
    // column-major host matrix -> row-major device T (streamed through a bounded staging buffer, column panels)
    void upload_matrix(const double* h, int64_t ldh, int rows, int cols, T* d, int64_t ldd) {
        if (rows <= 0 || cols <= 0) return;
        if (stage_mat && (int64_t)rows * cols <= stage_mat_count) {   // small matrix: one copy through the arena's staging area
            HIPC(hipMemcpy2DAsync(stage_mat, sizeof(double) * (size_t)rows, h, sizeof(double) * (size_t)ldh, sizeof(double) * (size_t)rows, (size_t)cols, hipMemcpyHostToDevice, st));
            import_colmajor<T>(st, stage_mat, rows, rows, cols, d, ldd);
            HIPC(hipStreamSynchronize(st));
            return;
        }
        upload_matrix_panels<T>(st, device, h, ldh, rows, cols, d, ldd);
    }

    DenseChol<T> chol() const { return {st, (int)n, NP, MP, P, A, PI, AA, M, S, tmp, dinv, fail}; }
    // LinSysSolInit: LinearSystemSolvers.jl:110-122 (mAA, mPI, mL) + factorisation (ProxQP.jl:196)
    void factorize(double rho, double sigma, bool rebuild_all) {
        const bool rebuild = rebuild_all || !have_AA;
        const DenseChol<T> c = chol();
        factor_valid = false; wh.invalidate();
        c.form(sigma, rho, rebuild, rebuild);                                                      // :112-114 / :128
        have_AA = true;
        c.factor(nb, 1, use_blocked());
        char ctx[128]; snprintf(ctx, sizeof ctx, "rho=%g, sigma=%g; factorisation #%d of this handle", rho, sigma, ++num_factorizations);
        int f = 0;
        c.check("P + sigma I + rho A'A", ctx, &f);
        factor_valid = true; fac_rho = rho; fac_sigma = sigma; fac_nb = nb; fac_premul = use_blocked();
    }
    // Did a blocked-sweep launch give up waiting (its workgroups were not co-resident: ANY concurrent work on the card can do that, other streams of
    // this process included -- the sweep gate chains the blocked sweeps only)?  Then the iterates are garbage: the caller repeats its work on the
    // multi-launch sweeps (`blocked_off` until the next solve / linsys_init), so a blocked-sweep solve is bit-reproducible only when it reports
    // sweepGaveUp == 0.  Synchronises the stream.
    bool sweep_gave_up(bool fetched = false) {
        if (!fac_premul) return false;
        unsigned* h = reinterpret_cast<unsigned*>(res_host + 14);
        if (!fetched) {
            HIPC(hipMemcpyAsync(h, abort_dev, sizeof(unsigned), hipMemcpyDeviceToHost, st));
            HIPC(hipStreamSynchronize(st));
        }
        if (*h == 0u) return false;
        HIPC(hipMemsetAsync(abort_dev, 0, sizeof(unsigned), st));
        blocked_off = true; factor_valid = false;
        return true;
    }

    // the fused pass over one block first, then the single-launch blocked sweeps (5, at least two blocks), then the multi-launch sweeps
    int sweep_variant() const { const int v = chol_sweep_variant<T>(NP, nb); return (fac_premul && v != 2) ? 5 : v; }
    // x~ = (L L')^{-1} tt via the blocked sweeps over S (tt is consumed)
    void sweeps() {
        if (sweep_variant() != 5) {
            chol().sweeps(nb, tt, yv, xx, sw_part, BatchStride(), {&prof, cat_sweep, sample_lvl(13), cat_xsum, sample_lvl(21), cat_fwd, cat_bwd, 2});
            return;
        }
        // blocked substitution, one launch per sweep: n / nb dependent phases handed from workgroup to workgroup inside the launch
        if (sweep_epoch >= 0xfffffff0u) {   // the granule tags are 32-bit launch counters: start over on a cleared buffer
            HIPC(hipMemsetAsync(pub, 0, sizeof(unsigned long long) * (size_t)trsv_blocked_pub_words<T>(NP), st));
            sweep_epoch = 0;
        }
        TrsvBlockedPair gate(device, st);   // never two of these persistent launches on the chip at once (k_trsv_blocked.hip, "Co-residency")
        { ProfLaunchScope ps(prof, cat_fwd, sample_lvl(13)); trsv_blocked<T>(st, false, S, NP, NP, nb, tt, yv, pub, ++sweep_epoch, abort_dev); }
        { ProfLaunchScope ps(prof, cat_bwd, sample_lvl(21)); trsv_blocked<T>(st, true, S, NP, NP, nb, yv, xx, pub, ++sweep_epoch, abort_dev); }
    }
    // LinSysSol! body: LinearSystemSolvers.jl:134-139
    void linear_solve(double rho, double sigma) {
        {
            ProfScope ps(prof, cat_atw, 1);
            gemv_cols_partial<T>(st, A, NP, z, y, (T)rho, T(-1), part, NP, MP, NP);                  // :134-135
        }
        {
            ProfScope ps(prof, cat_colsum, 2);
            colsum<T>(st, part, NP, part_tiles, x, (T)sigma, q, T(-1), tt, NP);                      // :136
        }
        sweeps();                                                                                   // :137 (Cholesky instead of cg!)
        {
            ProfScope ps(prof, cat_ax, 2);
            gemv_rows<T>(st, A, NP, xx, zz, nullptr, T(1), T(0), 0, MP, 0, NP, 0);                   // :139
        }
    }

    void solve(double* xh, const qps_params& p, qps_info* info) override {
        HIPC(hipSetDevice(device));
        blocked_off = false;                  // a handle whose launch gave up once tries the blocked sweeps again at every new solve
        int gave_up = 0; double t_lost = 0;
        const double t_begin = now_s();
        while (solve_once(xh, p, info)) {     // true: a blocked-sweep launch gave up; x on the host is still the caller's
            ++gave_up; t_lost = now_s() - t_begin;
            const int lvl = prof.level; prof.reset(); prof.level = lvl;   // the aborted attempt's launches are not this solve's kernels
        }
        if (info) { info->sweepGaveUp = gave_up; info->cgExplicit = 0; info->tLoop += t_lost; }   // the repeated work is loop time
    }
    // The three ADMM loops of a dense handle.  Each takes the loop state and returns what the epilogue reports.
    enum class Route { Small, Whitened, Classic };
    struct LoopEnd { int iterations; int variant; bool gave_up; };   // iterations done, qps_info.sweepVariant, a blocked sweep gave up (classic loop only)
    // Small: the whole loop in one single-workgroup launch.  Whitened: nothing was factorised in this call, fixed rho, the fused loop over one inverted block
    // (S lower = inv(L)) would run; B and G are built last, once per factor, when everything else holds (before the caller's t1: inside tSetup).  Neither of the
    // two runs with `fac_premul` set (one sweep block / the condition below), so neither has to ask sweep_gave_up().
    Route choose_route(const qps_params& p, bool reuse) {
        const bool small_path = small_ok && p.loopVariant == 0 && (NP + nb - 1) / nb == 1;
        const bool whiten = reuse && wh.wanted(NP) && !p.adptRho && m > 0 && p.loopVariant != 1 && pass_slabs > 0 && !small_path && !fac_premul &&
                            chol_sweep_variant<T>(NP, nb) != 1 && whitened_supported(NP, MP) && wh.build(whitened_view());
        return small_path ? Route::Small : whiten ? Route::Whitened : Route::Classic;
    }
    void drain() { HIPC(hipStreamSynchronize(st)); prof.harvest(); }
    // the read-back of a check: 15 doubles, slot 14 carries the blocked sweeps' give-up word (abort_dev)
    void fetch_check() { HIPC(hipMemcpyAsync(res_host, res_dev, 15 * sizeof(double), hipMemcpyDeviceToHost, st)); drain(); }
    bool solve_once(double* xh, const qps_params& p, qps_info* info) {
        if (p.linsys != QPS_LINSYS_AUTO && p.linsys != QPS_LINSYS_CHOLESKY)
            throw QpsError(QPS_ERR_UNSUPPORTED, "dense handles offer QPS_LINSYS_CHOLESKY only (qps_create_csc with dense_path = 0 for the CG and the sparse L D L' plugins)");
        const double t0 = now_s();
        nb = pick_nb<T>(p.trsvBlock, NP);
        AdmmLoop lp(p.rho);                                                                         // SolveQuadraticProgram.jl:33, :43
        const bool reuse = p.reuseFactor && factor_valid && fac_rho == lp.rho && fac_sigma == p.sigma && fac_nb == nb && fac_premul == use_blocked();
        if (!reuse) factorize(lp.rho, p.sigma, !p.reuseFactor || !have_AA || fac_sigma != p.sigma); // :36
        const Route route = choose_route(p, reuse);
        upload_vec(xh, x, n);
        HIPC(hipMemsetAsync(xp, 0, sizeof(T) * NP, st));                                            // :38
        HIPC(hipMemsetAsync(z, 0, sizeof(T) * std::max(MP, 64), st));                               // :39
        HIPC(hipMemsetAsync(y, 0, sizeof(T) * std::max(MP, 64), st));                               // :40
        HIPC(hipMemsetAsync(zp, 0, sizeof(T) * std::max(MP, 64), st));                              // :41
        HIPC(hipStreamSynchronize(st));
        const double t1 = now_s();
        LoopEnd end{};
        switch (route) {
        case Route::Small: end = loop_small(p, lp); break;
        case Route::Whitened: if constexpr (std::is_same<T, double>::value) end = loop_whitened(xh, p, lp); break;
        case Route::Classic: end = loop_classic(p, lp); break;
        }
        if (end.gave_up) return true;
        finish(xh, p, info, lp, end, t1 - t0, now_s() - t1);
        return false;
    }
    // the end of every route: polish, download, report (tLoop ended when the loop returned)
    void finish(double* xh, const qps_params& p, qps_info* info, const AdmmLoop& lp, const LoopEnd& end, double tSetup, double tLoop) {
        PolishReport pr;
        if (p.polish) polish_dense<T>(st, n, m, NP, MP, P, A, q, l, u, y, x, part, p, &pr);        // SolveQuadraticProgram.m:289-325
        download_vec(x, xh, n);
        if (!info) return;
        lp.fill_info(info, end.iterations, tSetup, tLoop, pr);
        info->cgIterations = 0; info->trsvBlock = nb; info->sweepVariant = end.variant;
    }
    // Small problem: the whole loop :45-71 runs inside one single-workgroup launch; the host only steps in for a rho switch.
    LoopEnd loop_small(const qps_params& p, AdmmLoop& lp) {
        transpose_small<T>(st, A, NP, MP, At);
        int it = 0;
        while (it < p.numIterations) {
            {
                ProfScope ps(prof, cat_small, 1);   // events around the one launch (a ~3 us launch gap against a kernel of hundreds of us)
                admm_small<T>(st, (int)n, (int)m, NP, MP, it, p.numIterations, p.numItrConv, p.adptRho, lp.rho, lp.rhorho, p.sigma, p.alpha, p.epsAbs,
                              p.epsRel, eps_admm(p), p.fctrRho, A, At, P, S, q, l, u, x, xp, z, y, small_out);
            }
            HIPC(hipMemcpyAsync(small_out_host, small_out, admm_small_out_bytes(), hipMemcpyDeviceToHost, st));
            drain();
            int last = 0, flag = 1, need = 0; double r8[8];
            admm_small_read(small_out_host, &last, &flag, &need, r8);
            it = last; lp.convFlag = flag; lp.rhorho = r8[4];
            if (!std::isnan(r8[0]) || !std::isnan(r8[1])) { lp.resP = r8[0]; lp.resD = r8[1]; }
            if (flag != QPS_CONV_NUM_ITR) break;                                                    // :66-68
            if (need && it < p.numIterations) refactor_at_switch(lp, p.sigma);                      // :47-51 (the loop top is never re-entered after the last iteration)
        }
        return {it, 4, false};
    }
    void refactor_at_switch(AdmmLoop& lp, double sigma) {                                           // :48-51
        lp.rho = lp.rhorho; ++lp.nref;
        const double ta = now_s();
        factorize(lp.rho, sigma, false);                                                            // changedΡ: LinearSystemSolvers.jl:127-129
        lp.tref += now_s() - ta;
    }
    // Whitened coordinates: u = W t, p = W x, a = A x.  x is formed from p = inv(L) x at a check and at the end only (x = L p).
    LoopEnd loop_whitened(const double* xh, const qps_params& p, AdmmLoop& lp) {
        static_assert(std::is_same<T, double>::value, "the whitened kernels are fp64 only");
        const WhitenedView<T> wv = whitened_view();
        T *pc = wh.p0, *pn = wh.p1;                                                                 // current p, and the buffer the next one goes to
        bool x0zero = true;
        for (int64_t i = 0; i < n && x0zero; ++i) x0zero = xh[i] == 0.0;
        if (x0zero) { HIPC(hipMemsetAsync(pc, 0, sizeof(T) * NP, st)); HIPC(hipMemsetAsync(wh.a, 0, sizeof(T) * MP, st)); }
        else {
            gemv_rows<T>(st, S, NP, x, pc, nullptr, T(1), T(0), 0, NP, 0, NP, 1);                   // p0 = W x0
            gemv_rows<T>(st, A, NP, x, wh.a, nullptr, T(1), T(0), 0, MP, 0, NP, 0);                 // a0 = A x0
        }
        gemv_rows<T>(st, S, NP, q, wh.c, nullptr, T(1), T(0), 0, NP, 0, NP, 1);                     // c = W q
        bool have_u = false;                                                                        // u of the next pass is formed (by a check's slab sum)
        auto slab_sum = [&](bool first, bool with_bty) {
            { ProfLaunchScope ps(prof, wh.cat_sum, sample_lvl(29)); whitened_sum(st, with_bty, wh.sum_args(NP, first, pc, pn, p.alpha, p.sigma)); }
            std::swap(pc, pn); have_u = true;
        };
        int ii;
        for (ii = 1; ii <= p.numIterations; ++ii) {                                                 // :45
            const bool check = (ii % p.numItrConv == 0);                                            // :63
            prof_iter = ii;
            if (!have_u) slab_sum(ii == 1, false);                                                  // :57 and LinearSystemSolvers.jl:134-137, multiplied by W
            if (check) HIPC(hipMemsetAsync(scratch, 0, 16 * sizeof(unsigned long long), st));
            {
                const int lvl = (prof.level == 1 && (check || ii % 50 != 38)) ? 3 : 1;              // sampled as the classic pass is
                ProfLaunchScope ps(prof, check ? wh.cat_passchk : wh.cat_pass, lvl);
                whitened_pass(st, check, wh.pass_args(wv, z, y, l, u, p.alpha, lp.rho, scratch));   // :59-61, :139, next :134-135; G u for :57
            }
            have_u = false;
            if (check) {
                slab_sum(false, true);                                                              // pc = p of this iteration, pn = the previous one
                { ProfScope ps(prof, wh.cat_l, 2); whitened_lpass(st, M, NP, NP, pc, pn, wh.bty, x, Aty, scratch); }   // x, |x - xp|, mA' * vY
                {
                    ProfScope ps(prof, cat_chk, 2);
                    gemv_rows<T>(st, P, NP, x, Px, nullptr, T(1), T(0), 0, NP, 0, NP, 0);            // mP * vX
                    check_convergence<T>(st, (int)n, (int)m, Ax, Px, Aty, q, x, xp, z, zp, scratch, res_dev, check_scalars(p, lp), 1);
                }
                fetch_check();
                lp.read_check(res_host);
                if (lp.convFlag != QPS_CONV_NUM_ITR) break;                                         // :66-68
            }
        }
        const int done = iterations_done(ii, p.numIterations);
        if (done > 0) {
            if (!have_u) slab_sum(false, false);
            gemv_rows<T>(st, M, NP, pc, x, nullptr, T(1), T(0), 0, NP, 0, NP, 1);                   // x = L p
        }
        drain();
        return {done, sweep_variant(), false};
    }
    static CheckScalars check_scalars(const qps_params& p, const AdmmLoop& lp) { return {p.epsAbs, p.epsRel, eps_admm(p), lp.rho, lp.rhorho, p.adptRho, lp.convFlag}; }
    // The classic loop: fused (eager or replayed as graphs) or unfused.  Swaps the members x and xp; the roles persist into the next solve (iter_graph is keyed on them).
    LoopEnd loop_classic(const qps_params& p, AdmmLoop& lp) {
        const double sigma = p.sigma, alpha = p.alpha;
        const bool fused = pass_slabs > 0 && p.loopVariant != 1;
        int rhs_slabs = 0;   // z = y = 0: A'(rho z - y) = 0, no slab to add for the first right-hand side
        // Launch-bound sizes (an iteration of four to eight kernels lasts less than the host needs to enqueue it): replay graphs.
        // Profiling brackets launches and stays eager.  (The blocked sweeps take a fresh epoch argument per launch: no replay.)
        const bool use_graph = fused && prof.level == 0 && p.numItrConv >= 3 && !fac_premul && (graph_env() >= 0 ? graph_env() != 0 : NP <= 2048);
        int ii;
        for (ii = 1; ii <= p.numIterations; ++ii) {                                                 // :45
            const bool changed = lp.wants_rho_switch(p);                                            // :47
            if (changed) refactor_at_switch(lp, sigma);
            const double rho = lp.rho;
            const bool check = (ii % p.numItrConv == 0);                                            // :63
            if (use_graph && !changed && !check && rhs_slabs == pass_slabs) {
                // the plain iterations up to the next check (an even number of them, so x / xp end in the same roles) as ONE graph launch
                int run = std::min(p.numItrConv - ii % p.numItrConv, p.numIterations - ii + 1) & ~1;
                hipGraphExec_t ge = run >= 2 ? iter_graph(run, x, xp, rho, sigma, alpha) : nullptr;
                if (ge) {
                    HIPC(hipGraphLaunch(ge, st));
                    ii += run - 1;
                    continue;
                }
            }
            if (!fused) {
                linear_solve(rho, sigma);                                                           // :54
                {
                    ProfScope ps(prof, cat_upd, 2);
                    admm_update<T>(st, NP, MP, xx, zz, x, xp, z, zp, y, l, u, (T)alpha, (T)rho);     // :56-61
                }
                if (check) {
                    ProfScope ps(prof, cat_chk, 2);
                    gemv_rows<T>(st, A, NP, x, Ax, nullptr, T(1), T(0), 0, MP, 0, NP, 0);            // mA * vX
                    gemv_rows<T>(st, P, NP, x, Px, nullptr, T(1), T(0), 0, NP, 0, NP, 0);            // mP * vX
                    gemv_cols_partial<T>(st, A, NP, y, nullptr, T(1), T(0), part, NP, MP, NP);       // mA' * vY
                    colsum<T>(st, part, NP, part_tiles, nullptr, T(0), nullptr, T(0), Aty, NP);
                    check_convergence<T>(st, (int)n, (int)m, Ax, Px, Aty, q, x, xp, z, zp, scratch, res_dev, check_scalars(p, lp));   // :64
                }
            } else {
                // Fused loop: the pass of iteration ii-1 already left the slabs of A'(rho z - y); after a rho switch they
                // are stale (w depends on rho) and are rebuilt by the plain column GEMV.
                if (changed && rhs_slabs > 0) {
                    ProfScope ps(prof, cat_atw, 2);
                    rhs_slabs = gemv_cols_partial<T>(st, A, NP, z, y, (T)rho, T(-1), part, NP, MP, NP);
                }
                prof_iter = ii;
                {
                    ProfLaunchScope ps(prof, cat_colsum, sample_lvl(29));
                    colsum<T>(st, part, NP, rhs_slabs, x, (T)sigma, q, T(-1), tt, NP);              // LinearSystemSolvers.jl:136
                }
                sweeps();                                                                           // :137
                if (check) HIPC(hipMemsetAsync(scratch, 0, 16 * sizeof(unsigned long long), st));
                {
                    // level 1 samples the dominant kernel on every 50th iteration only (an event pair per launch costs ~7 % of
                    // the loop, one in ten still ~3 %); level 2 brackets every launch of every kernel
                    const int lvl = (prof.level == 1 && (check || ii % 50 != 38)) ? 3 : 1;   // mid-chunk sample of the plain variant only
                    ProfLaunchScope ps(prof, check ? cat_passchk : cat_pass, lvl);   // the dispatch's own begin / end timestamps
                    apass<T>(st, check, A, NP, NP, MP, xx, x, xp, z, y, l, u, (T)alpha, (T)rho, part, part2, NP, scratch);
                }
                std::swap(x, xp);   // x now holds the relaxed iterate, xp the previous one (SolveQuadraticProgram.jl:56-57)
                rhs_slabs = pass_slabs;
                if (check) {
                    ProfScope ps(prof, cat_chk, 2);
                    colsum<T>(st, part2, NP, pass_slabs, nullptr, T(0), nullptr, T(0), Aty, NP);     // mA' * vY
                    gemv_rows<T>(st, P, NP, x, Px, nullptr, T(1), T(0), 0, NP, 0, NP, 0);            // mP * vX
                    check_convergence<T>(st, (int)n, (int)m, Ax, Px, Aty, q, x, xp, z, zp, scratch, res_dev, check_scalars(p, lp), 1);
                }
            }
            if (check) {
                fetch_check();
                if (sweep_gave_up(true)) return {0, 0, true};
                lp.read_check(res_host);
                if (lp.convFlag != QPS_CONV_NUM_ITR) break;                                         // :66-68
            }
        }
        drain();
        if (sweep_gave_up()) return {0, 0, true};
        return {iterations_done(ii, p.numIterations), sweep_variant(), false};
    }
    void polish(double* xh, const double* yh, const qps_params& p, qps_polish_report* rep) override {
        HIPC(hipSetDevice(device));
        upload_vec(xh, x, n); upload_vec(yh, y, m);
        PolishReport pr;
        polish_dense<T>(st, n, m, NP, MP, P, A, q, l, u, y, x, part, p, &pr);
        download_vec(x, xh, n);
        if (rep) to_c_report(pr, rep);
    }
    void get_dual(double* zh, double* yh) override {
        HIPC(hipSetDevice(device));
        if (zh) download_vec(z, zh, m);
        if (yh) download_vec(y, yh, m);
    }
    void linsys_init(double rho, double sigma, int linsys, int nbreq) override {
        HIPC(hipSetDevice(device));
        if (linsys != QPS_LINSYS_AUTO && linsys != QPS_LINSYS_CHOLESKY) throw QpsError(QPS_ERR_UNSUPPORTED, "dense handles support QPS_LINSYS_CHOLESKY only");
        nb = pick_nb<T>(nbreq, NP);
        blocked_off = false;
        factorize(rho, sigma, true);
    }
    void linsys_solve(const double* xh, const double* zh, const double* yh, double rho, double sigma, int changed,
                      double* xxh, double* zzh) override {
        HIPC(hipSetDevice(device));
        if (!factor_valid && !changed) throw QpsError(QPS_ERR_BAD_ARGUMENT, "qps_linsys_solve called before qps_linsys_init");
        if (changed) factorize(rho, sigma, false);                                                  // LinearSystemSolvers.jl:127-129
        upload_vec(xh, x, n); upload_vec(zh, z, m); upload_vec(yh, y, m);
        linear_solve(rho, sigma);
        if (sweep_gave_up()) { factorize(rho, sigma, false); linear_solve(rho, sigma); }
        download_vec(xx, xxh, n); download_vec(zz, zzh, m);
    }
    // qps_operator_apply: the GEMVs the loop and CheckConvergence use (SolveQuadraticProgram.jl:85-89), on work buffers only (x, z, y stay)
    void operator_apply(int op, const double* in, double* out, double rho, double sigma) override {
        HIPC(hipSetDevice(device));
        auto Pin = [&](T* dst) { gemv_rows<T>(st, P, NP, xx, dst, nullptr, T(1), T(0), 0, NP, 0, NP, 0); };
        auto Ain = [&](T* dst) { if (m > 0) gemv_rows<T>(st, A, NP, xx, dst, nullptr, T(1), T(0), 0, MP, 0, NP, 0); };
        auto Atv = [&](const T* v, T* dst) {
            if (m > 0) { gemv_cols_partial<T>(st, A, NP, v, nullptr, T(1), T(0), part, NP, MP, NP); colsum<T>(st, part, NP, part_tiles, nullptr, T(0), nullptr, T(0), dst, NP); }
            else HIPC(hipMemsetAsync(dst, 0, sizeof(T) * NP, st));
        };
        if (op == QPS_OP_AT) { upload_vec(in, zz, m); Atv(zz, Aty); download_vec(Aty, out, n); return; }
        upload_vec(in, xx, n);
        if (op == QPS_OP_P) { Pin(Px); download_vec(Px, out, n); }
        else if (op == QPS_OP_A) { Ain(Ax); download_vec(Ax, out, m); }
        else if (op == QPS_OP_PA) { Pin(Px); Ain(Ax); download_vec(Px, out, n); download_vec(Ax, out + n, m); }
        else if (op == QPS_OP_REDUCED) {                                                            // LinearSystemSolvers.jl:152-157
            Pin(Px); Ain(Ax); Atv(Ax, Aty);
            std::vector<double> a((size_t)n), b((size_t)n);
            download_vec(Px, a.data(), n); download_vec(Aty, b.data(), n);
            for (int64_t i = 0; i < n; ++i) out[i] = a[(size_t)i] + rho * b[(size_t)i] + sigma * in[i];
        } else throw QpsError(QPS_ERR_BAD_ARGUMENT, "unknown qps_operator_kind");
    }
};

}  // namespace

SolverBase* make_dense(int device, int64_t n, int64_t m, int dtype, const double* P, int64_t ldp, const double* A, int64_t lda,
                       const double* q, const double* l, const double* u) {
    auto load = [&](auto s) -> SolverBase* {   // a unique_ptr: a throw while loading drops the solver
        s->upload_matrix(P, ldp, (int)n, (int)n, s->P, s->NP);
        s->upload_matrix(A, lda, (int)m, (int)n, s->A, s->NP);
        s->upload_vec(q, s->q, n); s->upload_vec(l, s->l, m); s->upload_vec(u, s->u, m);
        return s.release();
    };
    if (dtype == QPS_F64) return load(std::make_unique<DenseSolver<double>>(device, n, m, dtype));
    return load(std::make_unique<DenseSolver<float>>(device, n, m, dtype));
}

}  // namespace qps
