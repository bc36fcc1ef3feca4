// qps_dense_batch.hip -- BatchedDenseSolver: the lock-step ADMM loop driver of a batch of independent dense QPs of one shape, behind make_dense_batch (qps_batch.h).
#include <memory>

#include "admm_loop.h"
#include "dense_chol.h"
#include "qps_batch.h"
#include "qps_internal.h"
#include "qps_kernels.h"
#include "qps_polish.h"

namespace qps {
namespace {

// =================================================================================================================
// Batch of independent dense QPs of one shape (BASELINE config 4).  All QPs advance in lock step through batched launches
// (blockIdx.y = QP); rho, the proposed rho, the convergence flag and the active mask are per QP, exactly as if each QP
// ran its own SolveQuadraticProgram! (the tests compare every QP of a batch with its own stand-alone run).
// =================================================================================================================
template <typename T> struct BatchedDenseSolver : BatchSolverBase {
    StreamLease lease; DeviceOwner mem; hipStream_t st = nullptr;   // destroyed in reverse: buffers, then the stream lease, then the base's Profiler
    int NP = 0, MP = 0, nb = 0, slabs = 0, rpw = 0, part_tiles = 0;
    T *A = nullptr, *P = nullptr, *q = nullptr, *l = nullptr, *u = nullptr, *PI = nullptr, *AA = nullptr, *M = nullptr, *S = nullptr,
      *tmp = nullptr, *dinv = nullptr;
    T *x = nullptr, *xp = nullptr, *xres = nullptr, *z = nullptr, *y = nullptr, *xx = nullptr, *tt = nullptr, *yv = nullptr, *part = nullptr,
      *part2 = nullptr, *part_tmp = nullptr, *sw_part = nullptr, *Px = nullptr, *Aty = nullptr;
    int* fail = nullptr; int* d_active = nullptr; double *d_rho = nullptr, *d_rhorho = nullptr;
    unsigned long long* scratch = nullptr; double* res_dev = nullptr; double* res_host = nullptr; double* stage = nullptr;
    int* h_int = nullptr; double* h_dbl = nullptr;   // pinned staging for the small per-QP arrays
    bool have_AA = false; double fac_sigma = -1; int fac_nb = -1; std::vector<double> fac_rho;   // per-QP factor cache
    char* sb_args = nullptr; void* sb_host = nullptr;                                              // small-batch path: argument / report slots
    int cat_pass = 0, cat_sweep = 0;
    static constexpr const char* kWhat = "P + sigma I + rho A'A";

    BatchedDenseSolver(int dev, int cnt, int64_t n_, int64_t m_) {
        device = dev; n = n_; m = m_; count = cnt;
        HIPC(hipSetDevice(device));
        st = prof.st = lease.acquire(device);
        NP = roundup(n, 64); MP = roundup(m, 64);
        slabs = apass_plan<T>(NP, MP, &rpw, count);
        {   // algorithmic bytes per launch of the batched kernels: `count` times the single-QP figures
            const double s = sizeof(T), c = cnt;
            cat_pass = prof.category("apass(fused A-pass, batched)", c * s * ((double)m * n + 3.0 * n + 6.0 * m));
            cat_sweep = prof.category("sweeps(fused fwd+bwd, batched, triangle read once)", c * s * ((double)n * (n + 1) / 2 + 2.0 * n));
        }
        part_tiles = gemv_cols_tiles(MP);
        const int64_t nn = (int64_t)NP * NP, c = count;
        A = mem.dalloc<T>(c * MP * NP, st); P = mem.dalloc<T>(c * nn, st); PI = mem.dalloc<T>(c * nn, st); AA = mem.dalloc<T>(c * nn, st); M = mem.dalloc<T>(c * nn, st);
        S = mem.dalloc<T>(c * nn, st); tmp = mem.dalloc<T>(c * nn, st); dinv = mem.dalloc<T>(c * (int64_t)(NP / 64) * 4096, st);
        q = mem.dalloc<T>(c * NP, st); l = mem.dalloc<T>(c * MP, st); u = mem.dalloc<T>(c * MP, st);
        x = mem.dalloc<T>(c * NP, st); xp = mem.dalloc<T>(c * NP, st); xres = mem.dalloc<T>(c * NP, st); xx = mem.dalloc<T>(c * NP, st); tt = mem.dalloc<T>(c * NP, st);
        yv = mem.dalloc<T>(c * NP, st); Px = mem.dalloc<T>(c * NP, st); Aty = mem.dalloc<T>(c * NP, st); z = mem.dalloc<T>(c * MP, st); y = mem.dalloc<T>(c * MP, st);
        // polishing (one QP at a time) writes the slabs of a count = 1 pass plan, or the tiles of the column GEMV, into `part`:
        // count * slabs can be smaller than either (count = 3, NP = 2048: 246 < 256)
        int rpw1 = 0;
        const int64_t part_slabs = std::max<int64_t>(std::max<int64_t>(c * slabs, apass_plan<T>(NP, MP, &rpw1, 1)), std::max(part_tiles, 1));
        part = mem.dalloc<T>(part_slabs * NP, st); part2 = mem.dalloc<T>(c * slabs * NP, st); part_tmp = mem.dalloc<T>((int64_t)std::max(part_tiles, 1) * NP, st);
        const int sw_slabs = sweep_fused_slabs<T>(NP, count); sw_part = mem.dalloc<T>(c * std::max(sw_slabs, 1) * NP, st);
        fail = mem.dalloc<int>(count + 4, st); d_active = mem.dalloc<int>(count + 4, st); d_rho = mem.dalloc<double>(count + 4, st); d_rhorho = mem.dalloc<double>(count + 4, st);
        scratch = mem.dalloc<unsigned long long>(16 * c, st); res_dev = mem.dalloc<double>(8 * c, st);
        res_host = mem.pinned<double>(8 * c); h_int = mem.pinned<int>(count + 4); h_dbl = mem.pinned<double>(2 * (count + 4));
        stage = mem.dalloc<double>(std::max<int64_t>((int64_t)MP * NP, nn) + 64, st);
    }
    ~BatchedDenseSolver() override {
        (void)hipSetDevice(device);
        (void)hipStreamSynchronize(st);
        prof.release_events();
    }
    // Loading a batch: everything goes through ONE pinned ring (several host threads fill a half while the other half travels) and ONE device staging buffer,
    // all on the handle's stream -- the copy into `stage` for matrix k + 1 is ordered behind the import kernel that read matrix k, so nothing waits on the host until
    // finish_loading().  (A synchronisation per matrix left the DMA idle while the host copied and the host idle while the DMA ran: 64 QPs of n = 1024 took 150 ms to load.)
    std::unique_ptr<FastUploader> loader;
    void put_vec(const double* h, T* d, int64_t cnt_) {
        if (cnt_ <= 0) return;
        if (!loader) loader.reset(new FastUploader(st, device));
        loader->copy(stage, h, sizeof(double) * (size_t)cnt_);
        convert_copy<T>(st, stage, d, cnt_);
    }
    void put_matrix(const double* h, int rows, int cols, T* d) {   // column-major rows x cols (ld = rows) -> row-major, ld NP
        if (rows <= 0 || cols <= 0) return;
        if (!loader) loader.reset(new FastUploader(st, device));
        loader->copy(stage, h, sizeof(double) * (size_t)rows * cols);
        import_colmajor<T>(st, stage, rows, rows, cols, d, NP);
    }
    void finish_loading() { HIPC(hipStreamSynchronize(st)); loader.reset(); }
    void get_dual(double* zh, double* yh) override {
        HIPC(hipSetDevice(device));
        for (int b = 0; b < count && m > 0; ++b) {
            if (zh) HIPC(download_staged<T>(st, stage, z + (int64_t)b * MP, zh + (int64_t)b * m, m));
            if (yh) HIPC(download_staged<T>(st, stage, y + (int64_t)b * MP, yh + (int64_t)b * m, m));
        }
    }
    void load_problem(int b, const double* Ph, const double* Ah, const double* qh, const double* lh, const double* uh) {
        put_matrix(Ph, (int)n, (int)n, P + (int64_t)b * NP * NP);
        put_matrix(Ah, (int)m, (int)n, A + (int64_t)b * MP * NP);
        put_vec(qh, q + (int64_t)b * NP, n); put_vec(lh, l + (int64_t)b * MP, m); put_vec(uh, u + (int64_t)b * MP, m);
    }
    // LinearSystemSolvers.jl:112-114 / :127-129: chol() covers the whole batch (every launch of the panel chain carries all QPs), chol().at(b) QP b alone;
    // no host synchronisation until its check() reads the fail words
    DenseChol<T> chol() const { return {st, (int)n, NP, MP, P, A, PI, AA, M, S, tmp, dinv, fail}; }
    void push_state(const std::vector<double>& rho, const std::vector<double>& rhorho, const std::vector<int>& active) {
        for (int b = 0; b < count; ++b) { h_dbl[b] = rho[b]; h_dbl[count + 4 + b] = rhorho[b]; h_int[b] = active[b]; }
        HIPC(hipMemcpyAsync(d_rho, h_dbl, sizeof(double) * count, hipMemcpyHostToDevice, st));
        HIPC(hipMemcpyAsync(d_rhorho, h_dbl + count + 4, sizeof(double) * count, hipMemcpyHostToDevice, st));
        HIPC(hipMemcpyAsync(d_active, h_int, sizeof(int) * count, hipMemcpyHostToDevice, st));
        HIPC(hipStreamSynchronize(st));   // the pinned staging is reused
    }

    // LinearSystemSolvers.jl:127-129 for the QPs of `changed`, whose rho[b] moved: one batched re-factorisation when at least half of the batch switches at this
    // check, else those QPs one by one.  `rebuild_slabs`: the slabs of A'(rho z - y) that the last pass left are stale and are rebuilt per QP;
    // `push_after`: the device copies of rho / rhorho / active are refreshed afterwards (push_state synchronises the stream).
    void refactor_changed(const std::vector<int>& changed, double sigma, const std::vector<double>& rho, const std::vector<double>& rhorho,
                          const std::vector<int>& active, std::vector<double>& tref, bool rebuild_slabs, bool push_after) {
        const double ta = now_s();
        const DenseChol<T> ch = chol();
        const bool together = (int)changed.size() * 2 >= count;   // most QPs switch at the same check: one batched refactor
        if (together) {
            push_state(rho, rhorho, active);                      // d_rho must hold the new values before assembly
            ch.form(sigma, 0.0, false, false, count, d_rho);
            ch.factor(nb, count);
            for (int b = 0; b < count; ++b) fac_rho[b] = rho[b];
        }
        for (int b : changed) {
            if (!together) { ch.at(b).form(sigma, rho[b], false, false); ch.at(b).factor(nb); fac_rho[b] = rho[b]; }
            if (rebuild_slabs) {   // slabs of A'(rho z - y) depend on rho: rebuild them for this QP (slab 0 = the sum, rest 0)
                T* pb_ = part + (int64_t)b * slabs * NP;
                gemv_cols_partial<T>(st, A + (int64_t)b * MP * NP, NP, z + (int64_t)b * MP, y + (int64_t)b * MP, (T)rho[b], T(-1), part_tmp, NP, MP, NP);
                colsum<T>(st, part_tmp, NP, part_tiles, nullptr, T(0), nullptr, T(0), pb_, NP);
                if (slabs > 1) HIPC(hipMemsetAsync(pb_ + NP, 0, sizeof(T) * (size_t)(slabs - 1) * NP, st));
            }
        }
        std::vector<int> all(count);
        for (int b = 0; b < count; ++b) all[b] = b;
        ch.check(kWhat, "", h_int, count, together ? &all : &changed);
        if (push_after) push_state(rho, rhorho, active);
        const double dt = (now_s() - ta) / changed.size();
        for (int b : changed) tref[b] += dt;
    }

    void solve_batch(double* xh, const qps_params& p, qps_info* infos) override {
        HIPC(hipSetDevice(device));
        const double t0 = now_s();
        if (slabs <= 0) throw QpsError(QPS_ERR_UNSUPPORTED, "batched path needs m >= 1 and n within the fused-pass limit");
        nb = pick_nb<T>(p.trsvBlock, NP);
        const DenseChol<T> ch = chol();
        const double sigma = p.sigma, alpha = p.alpha;
        const double epsAdmm = std::fmin(p.epsAbs, p.epsRel) * 1e-2;
        std::vector<double> rho(count, p.rho), rhorho(count, p.rho), resP(count, NAN), resD(count, NAN), tref(count, 0.0);
        std::vector<int> active(count, 1), conv(count, QPS_CONV_NUM_ITR), iters(count, p.numIterations), nref(count, 0);
        HIPC(hipMemsetAsync(fail, 0, sizeof(int) * count, st));
        const bool rebuild = !(p.reuseFactor && have_AA && fac_sigma == sigma);
        if ((int)fac_rho.size() != count) fac_rho.assign(count, -1.0);
        std::vector<int> todo;
        for (int b = 0; b < count; ++b)                                                             // SolveQuadraticProgram.jl:36
            if (rebuild || fac_rho[b] != p.rho || fac_nb != nb) todo.push_back(b);
        if ((int)todo.size() == count) { ch.form(sigma, p.rho, rebuild, rebuild, count); ch.factor(nb, count); }
        else for (int b : todo) { ch.at(b).form(sigma, p.rho, rebuild, rebuild); ch.at(b).factor(nb); }
        ch.check(kWhat, "", h_int, count, &todo);
        have_AA = true; fac_sigma = sigma; fac_nb = nb;
        for (int b : todo) fac_rho[b] = p.rho;
        for (int b = 0; b < count; ++b) put_vec(xh + (int64_t)b * n, x + (int64_t)b * NP, n);
        loader.reset();                                                                             // (gives the pinned ring back)
        HIPC(hipMemsetAsync(z, 0, sizeof(T) * (size_t)count * MP, st));                             // :39
        HIPC(hipMemsetAsync(y, 0, sizeof(T) * (size_t)count * MP, st));                             // :40
        push_state(rho, rhorho, active);
        const double t1 = now_s();
        BatchStride bsS; bsS.count = count; bsS.mat = (int64_t)NP * NP; bsS.vin = NP; bsS.vout = NP; bsS.active = d_active;
        BatchStride bsC; bsC.count = count; bsC.mat = (int64_t)slabs * NP; bsC.vin = NP; bsC.vout = NP; bsC.active = d_active;
        BatchStride bsK; bsK.count = count; bsK.vin = NP; bsK.vout = MP; bsK.active = d_active;
        PassBatch pb; pb.count = count; pb.slabs = slabs; pb.rho_arr = d_rho; pb.active = d_active;
        int rhs_slabs = 0, nactive = count, ii = 0;
        const int nblk = (NP + nb - 1) / nb;
        if (p.loopVariant == 0 && nblk == 1 && admm_small_batch_supported<T>(NP, MP)) {
            // Small shapes: ONE workgroup per QP runs that QP's whole loop (register-resident kernel, k_small.hip); the host only
            // steps in when some QP wants a rho switch (refactor, relaunch from its own iteration) -- SolveQuadraticProgram.jl:45-71 per QP.
            const size_t ab = admm_small_args_bytes(), ob = admm_small_out_bytes();
            if (!sb_host) { sb_args = mem.dalloc<char>((int64_t)(ab + ob) * count + 64, st); sb_host = mem.pinned<char>((ab + ob) * (size_t)count + 64); }
            char* args_h = static_cast<char*>(sb_host); char* outs_h = args_h + ab * count;
            char* args_d = sb_args; char* outs_d = sb_args + ab * count;
            std::vector<int> it(count, 0);
            HIPC(hipMemsetAsync(xp, 0, sizeof(T) * (size_t)count * NP, st));                        // :38
            while (nactive > 0) {
                for (int b = 0; b < count; ++b)
                    admm_small_args_set(args_h, b, (int)n, (int)m, NP, MP, it[b], active[b] ? p.numIterations : it[b], p.numItrConv, p.adptRho, rho[b], rhorho[b],
                                        sigma, alpha, p.epsAbs, p.epsRel, epsAdmm, p.fctrRho);
                HIPC(hipMemcpyAsync(args_d, args_h, ab * count, hipMemcpyHostToDevice, st));
                admm_small_batch<T>(st, count, NP, MP, args_d, A, P, S, q, l, u, x, xp, z, y, outs_d);
                HIPC(hipMemcpyAsync(outs_h, outs_d, ob * count, hipMemcpyDeviceToHost, st));
                HIPC(hipStreamSynchronize(st));
                std::vector<int> changed;
                for (int b = 0; b < count; ++b) {
                    if (!active[b]) continue;
                    int last = 0, flag = QPS_CONV_NUM_ITR, need = 0; double r8[8];
                    admm_small_read(outs_h + ob * b, &last, &flag, &need, r8);
                    it[b] = last; rhorho[b] = r8[4];
                    if (!std::isnan(r8[0]) || !std::isnan(r8[1])) { resP[b] = r8[0]; resD[b] = r8[1]; }
                    if (flag != QPS_CONV_NUM_ITR) { conv[b] = flag; iters[b] = last; active[b] = 0; --nactive; }   // :66-68
                    else if (need && last < p.numIterations) { rho[b] = rhorho[b]; ++nref[b]; changed.push_back(b); }   // :47-51
                    else { iters[b] = p.numIterations; active[b] = 0; --nactive; }
                }
                if (!changed.empty()) refactor_changed(changed, sigma, rho, rhorho, active, tref, false, false);   // (no push_state afterwards: it would drain the stream once more)
            }
            HIPC(hipMemcpyAsync(xres, x, sizeof(T) * (size_t)count * NP, hipMemcpyDeviceToDevice, st));
        }
        for (ii = 1; ii <= p.numIterations && nactive > 0; ++ii) {                                  // :45
            std::vector<int> changed;
            if (p.adptRho)
                for (int b = 0; b < count; ++b)
                    if (active[b] && wants_rho_switch(p, rho[b], rhorho[b])) {                       // :47
                        rho[b] = rhorho[b]; ++nref[b]; changed.push_back(b);
                    }
            if (!changed.empty()) refactor_changed(changed, sigma, rho, rhorho, active, tref, rhs_slabs > 0, true);
            const bool check = (ii % p.numItrConv == 0);
            colsum<T>(st, part, NP, rhs_slabs, x, (T)sigma, q, T(-1), tt, NP, bsC);                  // LinearSystemSolvers.jl:136
            ch.sweeps(nb, tt, yv, xx, sw_part, bsS, {&prof, cat_sweep, (prof.level == 1 && ii % 50 == 13) ? 1 : 2});   // :137
            if (check) HIPC(hipMemsetAsync(scratch, 0, 16 * sizeof(unsigned long long) * count, st));
            {
                ProfLaunchScope ps(prof, cat_pass, (prof.level == 1 && !check && ii % 50 == 38) ? 1 : (check ? 3 : 2));   // level 1: one plain launch in 50
                apass<T>(st, check, A, NP, NP, MP, xx, x, xp, z, y, l, u, (T)alpha, T(1), part, part2, NP, scratch, pb);   // :56-61 + next rhs
            }
            std::swap(x, xp);
            rhs_slabs = slabs;
            if (check) {                                                                            // :63-69
                colsum<T>(st, part2, NP, slabs, nullptr, T(0), nullptr, T(0), Aty, NP, bsC);
                BatchStride bsP = bsS; bsP.mat = (int64_t)NP * NP;
                gemv_rows<T>(st, P, NP, x, Px, nullptr, T(1), T(0), 0, NP, 0, NP, 0, bsP);
                CheckScalars cs{p.epsAbs, p.epsRel, epsAdmm, 0.0, 0.0, p.adptRho, QPS_CONV_NUM_ITR};
                check_convergence<T>(st, (int)n, (int)m, (const T*)nullptr, Px, Aty, q, x, xp, z, z, scratch, res_dev, cs, 1, bsK, d_rho, d_rhorho);
                HIPC(hipMemcpyAsync(res_host, res_dev, 8 * sizeof(double) * count, hipMemcpyDeviceToHost, st));
                HIPC(hipStreamSynchronize(st));
                prof.harvest();
                for (int b = 0; b < count; ++b) {
                    if (!active[b]) continue;
                    const double* r = res_host + 8 * b;
                    resP[b] = r[0]; resD[b] = r[1]; rhorho[b] = r[4]; conv[b] = (int)r[5];
                    if (conv[b] != QPS_CONV_NUM_ITR) {
                        active[b] = 0; iters[b] = ii; --nactive;
                        HIPC(hipMemcpyAsync(xres + (int64_t)b * NP, x + (int64_t)b * NP, sizeof(T) * NP, hipMemcpyDeviceToDevice, st));
                    }
                }
                push_state(rho, rhorho, active);
            }
        }
        for (int b = 0; b < count; ++b)
            if (active[b]) HIPC(hipMemcpyAsync(xres + (int64_t)b * NP, x + (int64_t)b * NP, sizeof(T) * NP, hipMemcpyDeviceToDevice, st));
        HIPC(hipStreamSynchronize(st));
        prof.harvest();
        const double t2 = now_s();
        std::vector<PolishReport> pol(count);
        if (p.polish)                                                                               // SolveQuadraticProgram.m:289-325, one QP after the other
            for (int b = 0; b < count; ++b)
                polish_dense<T>(st, n, m, NP, MP, P + (int64_t)b * NP * NP, A + (int64_t)b * MP * NP, q + (int64_t)b * NP, l + (int64_t)b * MP,
                                u + (int64_t)b * MP, y + (int64_t)b * MP, xres + (int64_t)b * NP, part, p, &pol[b]);
        for (int b = 0; b < count; ++b) {
            HIPC(download_staged<T>(st, stage, xres + (int64_t)b * NP, xh + (int64_t)b * n, n));
            if (infos) {
                qps_info& in = infos[b];
                in.convFlag = conv[b]; in.iterations = iters[b]; in.numRefactor = nref[b]; in.cgIterations = 0;
                in.rhoFinal = rho[b]; in.rhoProposed = rhorho[b]; in.resPrim = resP[b]; in.resDual = resD[b];
                in.tSetup = t1 - t0; in.tLoop = t2 - t1; in.tRefactor = tref[b];   // wall time of the whole batch
                in.polishFlag = pol[b].flag; in.polishIterations = pol[b].minresIterations; in.tPolish = pol[b].seconds;
                in.trsvBlock = nb; in.sweepVariant = chol_sweep_variant<T>(NP, nb);
                in.sweepGaveUp = 0; in.cgExplicit = 0;
            }
        }
    }
};

}  // namespace

BatchSolverBase* make_dense_batch(int device, int dtype, int count, int64_t n, int64_t m, const double* P, const double* A, const double* q, const double* l,
                                  const double* u) {
    int rpw = 0;
    const int NP = roundup(n, 64), MP = roundup(m, 64);
    if (!(count > 1 && m > 0 && (dtype == QPS_F64 ? apass_plan<double>(NP, MP, &rpw, count) : apass_plan<float>(NP, MP, &rpw, count)) > 0)) return nullptr;
    auto load = [&](auto s) -> BatchSolverBase* {   // a unique_ptr: a throw while loading drops the solver
        for (int64_t b = 0; b < count; ++b) s->load_problem((int)b, P + b * n * n, A + b * m * n, q + b * n, l + b * m, u + b * m);
        s->finish_loading();
        return s.release();
    };
    if (dtype == QPS_F64) return load(std::make_unique<BatchedDenseSolver<double>>(device, count, n, m));
    return load(std::make_unique<BatchedDenseSolver<float>>(device, count, n, m));
}

}  // namespace qps
