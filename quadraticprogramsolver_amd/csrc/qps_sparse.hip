// qps_sparse.hip -- SparseSolver: the ADMM driver of a CSC handle (SolveQuadraticProgram.jl:36-80 on SparseMatrixCSC inputs).
//
// Composed from the matrix set and the CG plugin of qps_spmv.h (kernels: k_sparse.hip) and the direct KKT plugin of qps_ldl.h (kernels: k_ldl.hip); its own
// state is the ADMM vectors, the plugin choice and the graph cache of the direct plugin's plain iteration.
#include <algorithm>

#include "admm_loop.h"
#include "qps_internal.h"
#include "qps_kernels.h"
#include "qps_ldl.h"
#include "qps_polish.h"
#include "qps_spmv.h"

namespace qps {

namespace {

template <typename T> struct SparseSolver : SolverBase {
    // destroyed in reverse: what works on the stream (the factor of `kkt`; the graphs go in the destructor body), `cgp` (names only), then inside `mats` the
    // buffers and the stream lease, then the base's Profiler -- also when the constructor throws half way
    SparseMatrices<T> mats; CgPlugin<T> cgp; KktPlugin<T> kkt;
    T *q = nullptr, *l = nullptr, *u = nullptr, *x = nullptr, *xp = nullptr, *z = nullptr, *zp = nullptr, *y = nullptr;
    T *xx = nullptr, *zz = nullptr, *w = nullptr, *tt = nullptr;
    T *Ax = nullptr, *Px = nullptr, *Aty = nullptr;
    unsigned long long* scratch = nullptr; double* res_dev = nullptr;
    int cat_spmv, cat_vec, cat_chk, cat_ldl;
    int plugin_kind = QPS_LINSYS_CG;
    // hipGraph replay of ONE plain iteration of the direct plugin (a dozen launches of 2-3 us of work each: the eager loop is bound by
    // the host's launch rate).  Keyed by the scalars baked into the kernel arguments; every pointer of the loop is fixed.
    struct IterGraph { double rho, sigma, alpha; hipGraphExec_t exec; };
    std::vector<IterGraph> graphs; bool graphs_disabled = false;
    void drop_graphs() { for (auto& gr : graphs) (void)hipGraphExecDestroy(gr.exec); graphs.clear(); }
    hipGraphExec_t iter_graph(double rho, double sigma, double alpha) {
        for (auto& gr : graphs) if (gr.rho == rho && gr.sigma == sigma && gr.alpha == alpha) return gr.exec;
        if (graphs_disabled) return nullptr;
        if (graphs.size() >= 8) drop_graphs();
        hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr;
        if (hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) != hipSuccess) { (void)hipGetLastError(); graphs_disabled = true; return nullptr; }
        kkt.ldl->iterate(x, xp, q, z, zp, y, l, u, alpha, rho, sigma, true);                        // SolveQuadraticProgram.jl:54-61, right-hand side already in place
        // nothing was enqueued while capturing, so a failure here just means: run this handle's iterations eagerly from now on
        if (hipStreamEndCapture(st, &graph) != hipSuccess || graph == nullptr) { (void)hipGetLastError(); graphs_disabled = true; return nullptr; }
        const hipError_t e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        if (e != hipSuccess) { (void)hipGetLastError(); graphs_disabled = true; return nullptr; }
        graphs.push_back({rho, sigma, alpha, exec});
        return exec;
    }

    // Which plugin a request means on a CSC handle, with the direct one factorised.  QPS_LINSYS_AUTO is the reference's modeAuto rule
    // (SolveQuadraticProgram.jl:143-151, qps_linsys_auto) on this handle's sizes and non-zero counts, so that a C caller passing AUTO reaches the direct
    // KKT plugin exactly when the reference would; when the factor then does not fit the level-scheduled plugin (QPS_ERR_UNSUPPORTED from the analysis) an
    // AUTO request falls back to CG -- an EXPLICIT QPS_LINSYS_KKT_LDL request still fails loudly.  (Which form of CG serves a CG request: CgPlugin::resolve_cg.)
    int resolve_kind(int linsys, double rho, double sigma, bool force) {
        int kind = linsys;
        if (linsys == QPS_LINSYS_AUTO) kind = qps_linsys_auto(n, m, mats.P.nnz, mats.A.nnz, 1);
        if (kind != QPS_LINSYS_KKT_LDL) return cgp.resolve_cg(linsys, rho, sigma, kkt);
        if (kkt.unfit && linsys == QPS_LINSYS_AUTO) return cgp.resolve_cg(linsys, rho, sigma, kkt);
        try { kkt.prepare(rho, sigma, force); }
        catch (const QpsError& e) {
            if (linsys == QPS_LINSYS_AUTO && e.code == QPS_ERR_UNSUPPORTED) { kkt.unfit = true; return cgp.resolve_cg(linsys, rho, sigma, kkt); }
            throw;
        }
        return QPS_LINSYS_KKT_LDL;
    }

    SparseSolver(int dev, int64_t n_, int64_t m_, int dt, const int64_t* Pcp, const int64_t* Pri, const double* Pnz,
                 const int64_t* Acp, const int64_t* Ari, const double* Anz, const double* qh, const double* lh, const double* uh, int base)
        : mats(dev, n_, m_), cgp(mats, prof), kkt(mats.st, n_, m_) {
        device = dev; n = n_; m = m_; dtype = dt; sparse = true;
        st = prof.st = mats.st;
        if (Pcp[n] - base > 2000000000LL || Acp[n] - base > 2000000000LL) throw QpsError(QPS_ERR_BAD_DIMENSION, "more than 2^31 non-zeros");
        // canonical host copies first (sorted rows, duplicates summed, 0-based: a C caller's CSC need not be what Julia's sparse() guarantees);
        // they feed the CSR copies below and, later, the analysis of the L D L' plugin
        KktHostCsc& h = kkt.host;
        layout::canonical_csc(n, Pcp, Pri, Pnz, base, h.Pcp, h.Pri, h.Pnz);
        layout::canonical_csc(n, Acp, Ari, Anz, base, h.Acp, h.Ari, h.Anz);
        const int64_t pnnz = (int64_t)h.Pri.size(), annz = (int64_t)h.Ari.size();
        layout::CsrHost Ph, Ah, Ath;
        try {
            Ph = layout::csc_as_transposed_csr(n, n, h.Pcp, h.Pri, h.Pnz);      // P: CSC == CSR (symmetric, full storage): its columns are its rows
            layout::csc_to_csr_pair(m, n, h.Acp, h.Ari, h.Anz, Ah, Ath);        // rows of A by a counting sort; rows of A' are the columns of A == the CSC
        } catch (const std::length_error& ex) { throw QpsError(QPS_ERR_BAD_DIMENSION, ex.what()); }
        mats.load(Ph, Ah, Ath);
        cgp.build(Ph, Ah);
        DeviceOwner& mem = mats.mem;
        const int64_t nn = n + 64, mm = m + 64;
        q = mem.dalloc<T>(nn, st); x = mem.dalloc<T>(nn, st); xp = mem.dalloc<T>(nn, st); xx = mem.dalloc<T>(nn, st); tt = mem.dalloc<T>(nn, st);
        Px = mem.dalloc<T>(nn, st); Aty = mem.dalloc<T>(nn, st);
        l = mem.dalloc<T>(mm, st); u = mem.dalloc<T>(mm, st); z = mem.dalloc<T>(mm, st); zp = mem.dalloc<T>(mm, st); y = mem.dalloc<T>(mm, st); zz = mem.dalloc<T>(mm, st);
        w = mem.dalloc<T>(mm, st); Ax = mem.dalloc<T>(mm, st);
        scratch = mem.dalloc<unsigned long long>(16, st); res_dev = mem.dalloc<double>(16, st);
        mats.upload_vec(qh, q, n); mats.upload_vec(lh, l, m); mats.upload_vec(uh, u, m);
        const double s = sizeof(T);
        const Csr &A = mats.A, &At = mats.At, &P = mats.P;
        auto spmv_bytes = [&](const Csr& M, int cols) { return (double)M.nnz * (s + 4) + M.nrows * 4.0 + s * (M.nrows + cols); };
        cat_spmv = prof.category("spmv(A / A')", 0.5 * (spmv_bytes(A, (int)n) + spmv_bytes(At, (int)m)));
        cgp.cat_op = prof.category("cg_iteration(A u, P u + rho A'. + sigma u, axpys)", spmv_bytes(A, (int)n) + spmv_bytes(At, (int)m) + spmv_bytes(P, (int)n) + s * 10.0 * n);
        cat_vec = prof.category("admm_update", s * (3.0 * n + 7.0 * m));
        cat_chk = prof.category("check_convergence", spmv_bytes(A, (int)n) + spmv_bytes(At, (int)m) + spmv_bytes(P, (int)n));
        cat_ldl = prof.category("kkt_ldl_solve(rhs, level sweeps, dense tail, post)", 0.0);   // bytes are known once the factor exists
        // the dominant kernel of the CG path: the stacked [P; A] product (nnz * 12 + rows * 4 + s * (rows + cols))
        cgp.cat_pa = prof.category("spmv_blk([P;A] u, x block in LDS)", (double)(pnnz + annz) * (s + 4) + (double)(n + m) * 4.0 + s * (double)(n + m + n));
        cgp.cat_at = prof.category("spmv_blk(A' v, x block in LDS)", spmv_bytes(At, (int)m));
        // every fill and every upload above was enqueued on `st` (qps_internal.h, stream-ordering rule): nothing to wait for here
        mats.up.reset();
    }
    ~SparseSolver() override {
        (void)hipSetDevice(device);
        (void)hipStreamSynchronize(st);
        drop_graphs();
        prof.release_events();
    }

    // LinOpCg! body (LinearSystemSolvers.jl:176-181), or the direct KKT plugins' Sol! body (:37-40)
    void linear_solve(double rho, double sigma) {
        if (plugin_kind == QPS_LINSYS_KKT_LDL) {
            ProfScope ps(prof, cat_ldl, 2);
            kkt.ldl->solve(x, q, z, y, rho, sigma, xx, zz);
            return;
        }
        mats.axpby(m, (T)rho, z, T(-1), y, w);                                                      // :176
        {
            ProfScope ps(prof, cat_spmv, 2);
            if (m > 0) { SpmvEpilogue<T> e; e.add0 = x; e.b0 = (T)sigma; e.add1 = q; e.b1 = T(-1); mats.mul(mats.At, w, tt, e); }   // :177-178
            else mats.axpby(n, (T)sigma, x, T(-1), q, tt);
        }
        cgp.cg(rho, sigma, tt, xx);                                                                 // :179
        {
            ProfScope ps(prof, cat_spmv, 2);
            if (m > 0) mats.mul(mats.A, xx, zz);                                                    // :181
        }
    }

    void solve(double* xh, const qps_params& p, qps_info* info) override {
        HIPC(hipSetDevice(device));
        const double t0 = now_s();
        AdmmLoop lp(p.rho); const double sigma = p.sigma, alpha = p.alpha;
        cgp.eps_pcg = p.epsPcg; cgp.itr_pcg = p.numItrPcg;
        if (p.linsys == QPS_LINSYS_CHOLESKY) throw QpsError(QPS_ERR_UNSUPPORTED, "CSR handles offer QPS_LINSYS_CG, QPS_LINSYS_CG_EXPLICIT and QPS_LINSYS_KKT_LDL (create with dense_path=1 for the reduced Cholesky path)");
        plugin_kind = resolve_kind(p.linsys, lp.rho, sigma, !p.reuseFactor);                        // SolveQuadraticProgram.jl:36 LinSysSolInit (incl. the factorisation)
        mats.upload_vec(xh, x, n);
        const size_t nb_ = sizeof(T) * (size_t)(n + 64), mb_ = sizeof(T) * (size_t)(m + 64);
        HIPC(hipMemsetAsync(xp, 0, nb_, st)); HIPC(hipMemsetAsync(xx, 0, nb_, st));                 // LinOpCgInit: vXX = zeros (:147)
        HIPC(hipMemsetAsync(z, 0, mb_, st)); HIPC(hipMemsetAsync(y, 0, mb_, st)); HIPC(hipMemsetAsync(zp, 0, mb_, st));
        HIPC(hipStreamSynchronize(st));
        const double t1 = now_s();
        int ii = 0;
        cgp.cg_total = 0; cgp.last_cg = 4;
        const int NPv = (int)n, MPv = (int)m;
        const bool use_graph = plugin_kind == QPS_LINSYS_KKT_LDL && prof.level == 0 && graph_env() != 0;
        bool ldl_rhs_ready = false;   // the fused post/update launch leaves the next right-hand side behind; stale after a rho switch
        double* const res_host = mats.check_host();
        for (ii = 1; ii <= p.numIterations; ++ii) {
            if (lp.wants_rho_switch(p)) {
                lp.rho = lp.rhorho; ++lp.nref;                                                      // matrix-free CG: nothing to rebuild
                if (plugin_kind == QPS_LINSYS_CG && cgp.cg_explicit) { const double ta = now_s(); cgp.reduced_values(lp.rho, sigma); lp.tref += now_s() - ta; }   // changedΡ: LinearSystemSolvers.jl:127-129
                if (plugin_kind == QPS_LINSYS_KKT_LDL) { const double ta = now_s(); kkt.prepare(lp.rho, sigma, true); lp.tref += now_s() - ta; ldl_rhs_ready = false; }   // changedΡ: numeric refactor only
            }
            const double rho = lp.rho;
            if (plugin_kind == QPS_LINSYS_KKT_LDL && prof.level < 2) {
                // direct plugin: sweeps + ONE launch for nu -> z~, the x / z / y updates and the next right-hand side (k_ldl_post_update)
                if (use_graph && ldl_rhs_ready && ii % p.numItrConv != 0) {
                    hipGraphExec_t ge = iter_graph(rho, sigma, alpha);
                    if (ge) { HIPC(hipGraphLaunch(ge, st)); continue; }                             // a plain iteration: same kernels, same order
                }
                kkt.ldl->iterate(x, xp, q, z, zp, y, l, u, alpha, rho, sigma, ldl_rhs_ready);
                ldl_rhs_ready = true;
            } else {
            linear_solve(rho, sigma);
            {
                ProfScope ps(prof, cat_vec, 2);
                admm_update<T>(st, NPv, MPv, xx, zz, x, xp, z, zp, y, l, u, (T)alpha, (T)rho);
            }
            }
            if (ii % p.numItrConv == 0) {
                {
                    ProfScope ps(prof, cat_chk, 2);
                    if (m > 0) mats.mul(mats.A, x, Ax);
                    mats.mul(mats.P, x, Px);
                    if (m > 0) mats.mul(mats.At, y, Aty);
                    else HIPC(hipMemsetAsync(Aty, 0, nb_, st));
                    CheckScalars cs{p.epsAbs, p.epsRel, eps_admm(p), rho, lp.rhorho, p.adptRho, lp.convFlag};
                    check_convergence<T>(st, (int)n, (int)m, Ax, Px, Aty, q, x, xp, z, zp, scratch, res_dev, cs);
                }
                HIPC(hipMemcpyAsync(res_host, res_dev, 8 * sizeof(double), hipMemcpyDeviceToHost, st));
                HIPC(hipStreamSynchronize(st));
                prof.harvest();
                lp.read_check(res_host);
                if (lp.convFlag != QPS_CONV_NUM_ITR) break;
            }
        }
        HIPC(hipStreamSynchronize(st));
        prof.harvest();
        const double t2 = now_s();
        PolishReport pr;
        if (p.polish) polish_device(p, &pr);
        mats.download_vec(x, xh, n);
        if (!info) return;
        lp.fill_info(info, iterations_done(ii, p.numIterations), t1 - t0, t2 - t1, pr);
        info->cgIterations = (int)cgp.cg_total; info->cgExplicit = (plugin_kind == QPS_LINSYS_CG && cgp.cg_explicit) ? 1 : 0;
        info->trsvBlock = 0; info->sweepVariant = 0; info->sweepGaveUp = 0;
    }
    void get_dual(double* zh, double* yh) override {
        HIPC(hipSetDevice(device));
        if (zh) mats.download_vec(z, zh, m);
        if (yh) mats.download_vec(y, yh, m);
    }
    // SolveQuadraticProgram.m:289-325 with the products of K as SpMVs (x block of length n, multiplier block of length m)
    void polish_device(const qps_params& p, PolishReport* pr) {
        PolishProduct<T> kmat = [&](const T* v, T delta, T* out, const T* mask, T* scratch) {
            { SpmvEpilogue<T> e; e.add0 = v; e.b0 = delta; mats.mul(mats.P, v, out, e); }           // P v_x + delta v_x
            if (m <= 0) return;
            mats.mul(mats.A, v, out + n);                                                           // A v_x
            polish_mask_rows<T>(st, (int)m, mask, v + n, delta, out + n, scratch);                  // mask . - delta mask v_lambda; scratch = mask v_lambda
            { SpmvEpilogue<T> e; e.add0 = out; e.b0 = T(1); mats.mul(mats.At, scratch, out, e); }   // + A'(mask v_lambda)
        };
        polish_with<T>(st, n, m, (int)n, (int)m, q, l, u, y, x, p, pr, kmat);
    }
    void polish(double* xh, const double* yh, const qps_params& p, qps_polish_report* rep) override {
        HIPC(hipSetDevice(device));
        mats.upload_vec(xh, x, n); mats.upload_vec(yh, y, m);
        PolishReport pr;
        polish_device(p, &pr);
        mats.download_vec(x, xh, n);
        if (rep) to_c_report(pr, rep);
    }
    // qps_operator_apply: one application of P / A / A' / [P; A] / the reduced operator (LinearSystemSolvers.jl:152-157) through the SpMV kernels the loop
    // uses for them; work buffers only (the CG plugin's cu, cc: n; tm: m; w: m), the solver state stays
    void operator_apply(int op, const double* in, double* out, double rho, double sigma) override {
        HIPC(hipSetDevice(device));
        T* const cu = cgp.cu; T* const cc = cgp.cc; T* const tm = cgp.tm;
        if (op == QPS_OP_AT) {
            mats.upload_vec(in, w, m);
            if (m > 0) mats.mul(mats.At, w, cc); else HIPC(hipMemsetAsync(cc, 0, sizeof(T) * (size_t)(n + 64), st));
            mats.download_vec(cc, out, n);
            return;
        }
        mats.upload_vec(in, cu, n);
        if (op == QPS_OP_P) { mats.mul(mats.P, cu, cc); mats.download_vec(cc, out, n); }
        else if (op == QPS_OP_A) { if (m > 0) mats.mul(mats.A, cu, tm); mats.download_vec(tm, out, m); }
        else if (op == QPS_OP_PA) {
            if (cgp.PA.blocked) {                                                                   // the stacked product of a CG iteration, then its blocks added up
                DeviceOwner tmp_mem;
                T* both = tmp_mem.dalloc<T>(n + m + 64, st);
                cgp.stacked_product(cu, both);
                mats.download_vec(both, out, n); mats.download_vec(both + n, out + n, m);
            } else {
                mats.mul(mats.P, cu, cc); mats.download_vec(cc, out, n);
                if (m > 0) mats.mul(mats.A, cu, tm);
                mats.download_vec(tm, out + n, m);
            }
        } else if (op == QPS_OP_REDUCED) { cgp.op_reduced(cu, cc, rho, sigma, nullptr, nullptr); mats.download_vec(cc, out, n); }
        else throw QpsError(QPS_ERR_BAD_ARGUMENT, "unknown qps_operator_kind");
    }
    void linsys_set_cg(double eps, int itr) override { cgp.eps_pcg = eps; cgp.itr_pcg = itr; }     // LinOpCg!(...; ϵPcg, numItrPcg): LinearSystemSolvers.jl:164
    void linsys_init(double rho, double sigma, int linsys, int) override {
        HIPC(hipSetDevice(device));
        if (linsys != QPS_LINSYS_AUTO && linsys != QPS_LINSYS_CG && linsys != QPS_LINSYS_KKT_LDL && linsys != QPS_LINSYS_CG_EXPLICIT)
            throw QpsError(QPS_ERR_UNSUPPORTED, "CSR handles offer QPS_LINSYS_CG, QPS_LINSYS_CG_EXPLICIT and QPS_LINSYS_KKT_LDL (create with dense_path=1 for the reduced Cholesky path)");
        plugin_kind = resolve_kind(linsys, rho, sigma, true);                                       // LinearSystemSolvers.jl:18 / :49 / :81
        if (plugin_kind == QPS_LINSYS_KKT_LDL) return;
        HIPC(hipMemsetAsync(xx, 0, sizeof(T) * (size_t)(n + 64), st));                              // LinOpCgInit (:147)
        cgp.cg_total = 0; cgp.last_cg = 4;
    }
    void linsys_solve(const double* xh, const double* zh, const double* yh, double rho, double sigma, int changed, double* xxh, double* zzh) override {
        HIPC(hipSetDevice(device));
        if (plugin_kind == QPS_LINSYS_KKT_LDL) {
            if (!kkt.ldl) throw QpsError(QPS_ERR_BAD_ARGUMENT, "qps_linsys_solve called before qps_linsys_init");
            if (changed) kkt.prepare(rho, sigma, true);                                             // :30-32 / :61-63 / :93-95
        }
        if (plugin_kind == QPS_LINSYS_CG && cgp.cg_explicit) cgp.reduced_values(rho, sigma);         // :127-129 (a no-op while rho and sigma are the cached ones)
        mats.upload_vec(xh, x, n); mats.upload_vec(zh, z, m); mats.upload_vec(yh, y, m);
        linear_solve(rho, sigma);
        HIPC(hipStreamSynchronize(st));
        mats.download_vec(xx, xxh, n); mats.download_vec(zz, zzh, m);
    }
};

}  // namespace

SolverBase* make_sparse_solver(int device, int64_t n, int64_t m, int dtype, const int64_t* Pcp, const int64_t* Pri,
                               const double* Pnz, const int64_t* Acp, const int64_t* Ari, const double* Anz, const double* q,
                               const double* l, const double* u, int index_base) {
    if (dtype == QPS_F64) return new SparseSolver<double>(device, n, m, dtype, Pcp, Pri, Pnz, Acp, Ari, Anz, q, l, u, index_base);
    return new SparseSolver<float>(device, n, m, dtype, Pcp, Pri, Pnz, Acp, Ari, Anz, q, l, u, index_base);
}

}  // namespace qps
