// qps_shared_dense.hip -- the dense path of the shared-matrix batches: SharedBatchSolver, the Cholesky on MFMA panels (k_shared.hip) under the family driver of
// qps_shared_family.h.  qps_capi.hip validates the caller's arrays and builds the handle through the factory at the end of this file.
#include "dense_chol.h"
#include "qps_shared_family.h"

namespace qps {
namespace {

// =================================================================================================================
// Dense path.  One copy of every matrix, one factorisation, one sweep matrix with a single inverted block; every product of the loop is a row-major matrix times
// panels on the MFMA pipe (k_shared.hip), so a matrix is read once per launch whatever `count` is.  Per iteration: A' (a row-major copy of the transpose), the
// lower and the upper triangle of S, A.  Panels are NP = roundup(n, 64) and MP = roundup(m, 64) rows long, zero padded.
// =================================================================================================================
template <typename T> struct SharedBatchSolver final : SharedFamilySolver<T> {
    using B = SharedFamilySolver<T>;
    using B::device; using B::n; using B::m; using B::prof; using B::mem; using B::st; using B::up; using B::CP; using B::npanel;
    using B::q; using B::l; using B::u; using B::x; using B::xp; using B::z; using B::zp; using B::y; using B::Ax; using B::Px; using B::Aty;
    using B::d_active; using B::h_int; using B::factor_valid; using B::fac_rho; using B::fac_sigma; using B::num_factorizations;
    using B::cat_chk; using B::cat_fac; using B::cat_switch; using B::cat_start; using B::rho_scale; using B::rs_rho; using B::rs_rho1;
    using B::kd; using B::ke; using B::eq_kd; using B::eq_ke;
    int NP = 0, MP = 0, nb = 0;
    T *A = nullptr, *At = nullptr, *P = nullptr, *PI = nullptr, *AA = nullptr, *M = nullptr, *S = nullptr, *tmp = nullptr, *dinv = nullptr;
    T *xx = nullptr, *tt = nullptr, *yv = nullptr, *w = nullptr;
    int* fail = nullptr; bool have_AA = false;
    bool pi_stale = false;   // qps_update_shared_matrices replaced P alone: PI = P + sigma I is rebuilt at the next factorisation, the cached A'A is not
    int cat_atw = 0, cat_fwd = 0, cat_bwd = 0, cat_pass = 0;
    // The per-row rho scale here: Ws = diag(sqrt(s_i)) A (MP x NP) stands in for A when A'A is formed, so M = PI + rho Ws'Ws comes out of the same symmetric
    // product and a change of the base rho alone only re-assembles.  Equilibration: At holds D A' E beside D P D and E A D.
    T *Ws = nullptr, *rs_sqrt = nullptr;
    PanelArgs<T> a_rhs, a_fwd, a_bwd, a_row; SharedPanelOp op_row = SharedPanelOp::rows_zy;   // the launches of the running solve

    SharedBatchSolver(int dev, int cnt, int64_t n_, int64_t m_) : B(dev, cnt, n_, m_, roundup(n_, 64), roundup(m_, 64)) {
        NP = this->rowsN; MP = this->rowsM;
        this->info_trsv_block = nb = pick_nb<T>(32768, NP);   // one inverted block over the whole factor
        this->info_sweep_variant = 3;
        const int64_t nn = (int64_t)NP * NP, mn = (int64_t)MP * NP, pn = (int64_t)CP * NP, pm = (int64_t)CP * MP;
        A = mem.template dalloc<T>(mn, st); At = mem.template dalloc<T>(mn, st); P = mem.template dalloc<T>(nn, st); PI = mem.template dalloc<T>(nn, st);
        AA = mem.template dalloc<T>(nn, st); M = mem.template dalloc<T>(nn, st); S = mem.template dalloc<T>(nn, st); tmp = mem.template dalloc<T>(nn, st);
        dinv = mem.template dalloc<T>((int64_t)(NP / 64) * 4096, st);
        this->alloc_state_panels();
        xx = mem.template dalloc<T>(pn, st); tt = mem.template dalloc<T>(pn, st); yv = mem.template dalloc<T>(pn, st); w = mem.template dalloc<T>(pm, st);
        fail = mem.template dalloc<int>(4, st);
        // algorithmic bytes per launch: the matrix once, the panels it reads and writes
        const double s = sizeof(T), c = CP;
        cat_atw = prof.category("shared: A'w + rhs (MFMA panels)", s * ((double)m * n + c * (m + 3.0 * n)));
        cat_fwd = prof.category("shared: forward sweep (MFMA panels)", s * ((double)n * (n + 1) / 2 + 2.0 * c * n));
        cat_bwd = prof.category("shared: backward sweep + x (MFMA panels)", s * ((double)n * (n + 1) / 2 + 5.0 * c * n));
        cat_pass = prof.category("shared: A x~ + row updates (MFMA panels)", s * ((double)m * n + c * (n + 8.0 * m)));
        cat_chk = prof.category("shared: check (A x, P x, A'y, norms)", s * (2.0 * m * n + (double)n * n + c * (8.0 * n + 6.0 * m)));
        this->cat_inf = prof.category("shared: infeasibility (deltas, 3 products, sums)", s * (2.0 * m * n + (double)n * n + c * (10.0 * n + 10.0 * m)));
        cat_fac = prof.category("shared: factorisation at setup", s * ((double)m * n + 4.0 * n * n));
        cat_switch = prof.category("shared: rho switch (assemble, Cholesky, w)", s * (3.0 * n * n + 3.0 * c * m));
        cat_start = prof.category("shared: warm start (w, or A x -> z, w)", s * 3.0 * c * m);
    }
    ~SharedBatchSolver() override { this->drain(); }
    void load(const double* Ph, int64_t ldp, const double* Ah, int64_t lda, const double* qh, const double* lh, const double* uh) {
        upload_matrix_panels<T>(st, device, Ph, ldp, (int)n, (int)n, P, NP);
        upload_matrix_panels<T>(st, device, Ah, lda, (int)m, (int)n, A, NP);
        transpose_rowmajor<T>(st, A, NP, MP, NP, At, MP);   // row-major A': every product of the loop is "row-major matrix x panel"
        this->update_vectors(qh, lh, uh);
    }
    bool takes_csc() const override { return false; }
    void update_matrices_csc(const CanonicalCsc&, const CanonicalCsc&) override {
        throw QpsError(QPS_ERR_UNSUPPORTED, "qps_update_shared_matrices_csc: a dense shared-matrix batch takes its matrices through qps_update_shared_matrices");
    }
    void get_pattern(int64_t*, int64_t*, int64_t*, int64_t*, int64_t*, int64_t*) override {
        throw QpsError(QPS_ERR_UNSUPPORTED, "qps_get_shared_pattern: a dense shared-matrix batch stores no sparsity pattern");
    }
    ValuesVerdict update_values(const double*, int64_t, const double*, int64_t, int) override {
        throw QpsError(QPS_ERR_UNSUPPORTED, "qps_update_shared_values: a dense shared-matrix batch takes its matrices through qps_update_shared_matrices");
    }
    // New P and / or A (column-major, validated by the caller) into the storage of the old ones, scaled by the kept exponents while the equilibration is on; q, l,
    // u, z, y, every option and every allocation stay.  The range of the scaled entries is checked on the host before the first upload.
    void update_matrices(const double* Ph, int64_t ldp, const double* Ah, int64_t lda) override {
        if (!Ph && !Ah) return;
        HIPC(hipSetDevice(device));
        HIPC(hipStreamSynchronize(st));
        if (kd) {
            const int nt = host_threads();
            std::vector<double> his((size_t)nt, 0.0), los((size_t)nt, INFINITY);
            host_parallel(n, 64, [&](int t, int64_t j0, int64_t j1) {
                double hi = 0, lo = INFINITY;
                for (int64_t j = j0; j < j1; ++j) {
                    for (int64_t i = 0; Ph && i < n; ++i) equil_range_add<T>(Ph[i + j * ldp], eq_kd[i] + eq_kd[j], hi, lo);
                    for (int64_t i = 0; Ah && i < m; ++i) equil_range_add<T>(Ah[i + j * lda], eq_ke[i] + eq_kd[j], hi, lo);
                }
                his[t] = hi; los[t] = lo;
            });
            equil_check_range<T>(*std::max_element(his.begin(), his.end()), *std::min_element(los.begin(), los.end()), "qps_update_shared_matrices");
        }
        if (Ph) {
            upload_matrix_panels<T>(st, device, Ph, ldp, (int)n, (int)n, P, NP);
            if (kd) scale_two_sided<T>(st, P, NP, NP, kd, kd, 1);
            pi_stale = true;
        }
        if (Ah) {
            upload_matrix_panels<T>(st, device, Ah, lda, (int)m, (int)n, A, NP);
            transpose_rowmajor<T>(st, A, NP, MP, NP, At, MP);
            if (kd) { scale_two_sided<T>(st, A, MP, NP, ke, kd, 1); scale_two_sided<T>(st, At, NP, MP, kd, ke, 1); }
            if (Ws) scale_rows<T>(st, A, rs_sqrt, MP, NP, Ws);         // the per-row rho scale reads the new A
            have_AA = false;                                           // the cached product belongs to the previous A
        }
        HIPC(hipStreamSynchronize(st));
        factor_valid = false;                                          // the next solve factorises, also with reuseFactor
        this->last_conv.clear();
    }
    // the matrices and every vector the handle keeps between calls, in place: *= 2^(+-k) by the exponents in kd / ke
    void apply_equilibration(int sign) {
        scale_two_sided<T>(st, P, NP, NP, kd, kd, sign);
        scale_two_sided<T>(st, A, MP, NP, ke, kd, sign);
        scale_two_sided<T>(st, At, NP, MP, kd, ke, sign);
        this->rescale_kept_vectors(sign);
    }
    void set_equilibration(int passes) override {
        HIPC(hipSetDevice(device));
        HIPC(hipStreamSynchronize(st));
        const bool was_on = kd != nullptr;
        if (was_on) apply_equilibration(-1);                       // the caller's matrices again, bit for bit
        int *nkd = nullptr, *nke = nullptr; std::vector<int> hkd, hke;
        if (passes > 0) {
            nkd = mem.template dalloc<int>(NP, st); nke = mem.template dalloc<int>(MP, st);
            double* nrm = mem.template dalloc<double>(3 * (int64_t)NP + 2 * (int64_t)MP, st);
            double *cnP = nrm, *cnA = nrm + NP, *rn = nrm + 2 * NP, *loP = nrm + 2 * NP + MP, *loA = nrm + 3 * NP + MP;
            for (int k = 0; k < passes; ++k) {                     // Jacobi: every norm of a pass reads the exponents from before the pass
                equil_rownorm<T>(st, P, NP, NP, nkd, nkd, cnP, nullptr);        // P is symmetric and At is kept row-major: every norm is a row reduction
                equil_rownorm<T>(st, At, NP, MP, nkd, nke, cnA, nullptr);
                equil_rownorm<T>(st, A, MP, NP, nke, nkd, rn, nullptr);
                equil_update(st, NP, cnP, cnA, nkd);
                equil_update(st, MP, rn, nullptr, nke);
            }
            equil_rownorm<T>(st, P, NP, NP, nkd, nkd, cnP, loP);
            equil_rownorm<T>(st, A, MP, NP, nke, nkd, rn, loA);
            std::vector<double> h(3 * (size_t)NP + 2 * (size_t)MP);
            hkd.resize(NP); hke.resize(MP);
            HIPC(hipMemcpyAsync(h.data(), nrm, sizeof(double) * h.size(), hipMemcpyDeviceToHost, st));
            HIPC(hipMemcpyAsync(hkd.data(), nkd, sizeof(int) * NP, hipMemcpyDeviceToHost, st));
            HIPC(hipMemcpyAsync(hke.data(), nke, sizeof(int) * MP, hipMemcpyDeviceToHost, st));
            HIPC(hipStreamSynchronize(st));
            mem.release(nrm);
            double hi = 0, lo = INFINITY;
            for (int i = 0; i < NP; ++i) { hi = std::fmax(hi, h[i]); lo = std::fmin(lo, h[2 * (size_t)NP + MP + i]); }
            for (int i = 0; i < MP; ++i) { hi = std::fmax(hi, h[2 * (size_t)NP + i]); lo = std::fmin(lo, h[3 * (size_t)NP + MP + i]); }
            try { equil_check_range<T>(hi, lo); }
            catch (...) {
                mem.release(nkd); mem.release(nke);
                if (was_on) { apply_equilibration(1); HIPC(hipStreamSynchronize(st)); }   // the previous scaling, its factor and its cached product stay
                throw;
            }
        }
        mem.release(kd); mem.release(ke);
        kd = nkd; ke = nke;
        eq_kd.assign(hkd.begin(), hkd.begin() + (passes > 0 ? n : 0)); eq_ke.assign(hke.begin(), hke.begin() + (passes > 0 ? m : 0));
        if (kd) apply_equilibration(1);
        if (Ws) scale_rows<T>(st, A, rs_sqrt, MP, NP, Ws);         // the per-row rho scale reads the new A
        HIPC(hipStreamSynchronize(st));
        factor_valid = false; have_AA = false;                     // the cached product and the factor belong to the previous matrices
        this->last_conv.clear();                                   // and a certificate to the scaling it was taken in
    }
    void rho_scale_changed(const double* s) override {
        if (!s) {
            for (T** v : {&Ws, &rs_sqrt}) { mem.release(*v); *v = nullptr; }
        } else {
            if (!Ws) Ws = mem.template dalloc<T>((int64_t)MP * NP, st);
            if (!rs_sqrt) rs_sqrt = mem.template dalloc<T>(MP, st);
            std::vector<T> h((size_t)MP, T(1));
            for (int64_t i = 0; i < m; ++i) h[i] = (T)std::sqrt(s[i]);
            up->copy(rs_sqrt, h.data(), sizeof(T) * (size_t)MP);
            scale_rows<T>(st, A, rs_sqrt, MP, NP, Ws);
            HIPC(hipStreamSynchronize(st));
        }
        factor_valid = false; have_AA = false;   // the cached product and the factor belong to the previous scale
    }
    // LinSysSolInit once for all columns: LinearSystemSolvers.jl:110-122 + factorisation, sweep matrix with one inverted block
    void factorize(double rho, double sigma, bool rebuild_all) {
        const bool rebuild = rebuild_all || !have_AA;
        const DenseChol<T> c{st, (int)n, NP, MP, P, rho_scale.empty() ? A : Ws, PI, AA, M, S, tmp, dinv, fail};   // A'A, or A' diag(s) A = Ws'Ws
        factor_valid = false;
        HIPC(hipMemsetAsync(fail, 0, sizeof(int) * 4, st));
        c.form(sigma, rho, rebuild || pi_stale, rebuild);
        have_AA = true; pi_stale = false;
        c.factor(nb);
        char ctx[128]; snprintf(ctx, sizeof ctx, "rho=%g, sigma=%g; factorisation #%d of this handle", rho, sigma, ++num_factorizations);
        c.check("P + sigma I + rho A'A", ctx, h_int);
        factor_valid = true; fac_rho = rho; fac_sigma = sigma;
    }
    PanelArgs<T> product_args(const T* Mat, int64_t ld, int rows, int K, const T* Bp, T* out) const {
        PanelArgs<T> a; a.Mat = Mat; a.ld = ld; a.rows = rows; a.K = K; a.B = Bp; a.npanel = npanel; a.out = out; a.active = d_active;
        return a;
    }

  protected:
    void check_params(const qps_params& p) override {
        if (p.adptRho) throw QpsError(QPS_ERR_UNSUPPORTED, "shared-matrix batch: adptRho is not supported (one factor serves every column, so the per-problem rule cannot run; "
                                                           "qps_set_shared_adaptive_rho turns on the family-wide rule)");
        if (p.polish) throw QpsError(QPS_ERR_UNSUPPORTED, "shared-matrix batch: polishing is not supported");
        if (p.trsvBlock != 0 && p.trsvBlock < n)
            throw QpsError(QPS_ERR_UNSUPPORTED, "shared-matrix batch: trsvBlock must be 0 or >= n (the sweeps run over one inverted block covering the whole factor)");
        if (p.linsys != QPS_LINSYS_AUTO && p.linsys != QPS_LINSYS_CHOLESKY) throw QpsError(QPS_ERR_UNSUPPORTED, "shared-matrix batch: QPS_LINSYS_CHOLESKY only");
    }
    void factor_at_setup(double rho, double sigma, const qps_params& p) override { factorize(rho, sigma, !p.reuseFactor || !have_AA || fac_sigma != sigma); }
    void begin_solve(int warm, double rho, double sigma, double alpha) override {
        const bool scaled = !rho_scale.empty();
        this->reset_state(warm);
        for (T* v : {xx, tt, yv}) HIPC(hipMemsetAsync(v, 0, sizeof(T) * (size_t)CP * NP, st));
        HIPC(hipMemsetAsync(w, 0, sizeof(T) * (size_t)CP * MP, st));
        this->push_active();
        if (warm == 1) {                                                                            // w = rho_i z - y for this solve's rho: what the row update would have left
            ProfScope ps(prof, cat_start, 1);
            panel_w<T>(st, z, y, d_active, scaled ? rs_rho : nullptr, (T)rho, MP, npanel, w);
        } else if (warm == 2) {                                                                     // OSQP's warm_start(x, y): z = A x~ without projection, w with the stored y
            ProfScope ps(prof, cat_start, 1);
            PanelArgs<T> a_st = product_args(A, NP, MP, NP, x, nullptr);
            a_st.z = z; a_st.y = y; a_st.w = w; a_st.rho = (T)rho; a_st.rho_row = scaled ? rs_rho : nullptr;
            shared_panel<T>(st, SharedPanelOp::start_z, a_st);
        }
        a_rhs = product_args(At, MP, NP, MP, w, tt); a_rhs.x = x; a_rhs.q = q; a_rhs.sigma = (T)sigma;
        a_fwd = product_args(S, NP, NP, NP, tt, yv);
        a_bwd = product_args(S, NP, NP, NP, yv, xx); a_bwd.x = x; a_bwd.xp = xp; a_bwd.alpha = (T)alpha;
        a_row = product_args(A, NP, MP, NP, xx, nullptr);
        a_row.z = z; a_row.zp = zp; a_row.y = y; a_row.w = w; a_row.l = l; a_row.u = u; a_row.alpha = (T)alpha; a_row.rho = (T)rho;
        a_row.rho_row = rs_rho; a_row.rho1_row = rs_rho1;
        op_row = scaled ? SharedPanelOp::rows_zy_scaled : SharedPanelOp::rows_zy;
    }
    void switch_rho(double rho, double sigma) override {
        const bool scaled = !rho_scale.empty();
        factorize(rho, sigma, false);                                                               // changedΡ: A'A is kept, assembly and Cholesky only
        if (scaled) this->push_row_rho(rho);
        a_row.rho = (T)rho;
        panel_w<T>(st, z, y, d_active, scaled ? rs_rho : nullptr, (T)rho, MP, npanel, w);           // w held rho z - y of the previous rho
    }
    void iterate(int lvl, double, double, double) override {   // rho, sigma and alpha travel in the launch arguments
        { ProfLaunchScope ps(prof, cat_atw, lvl); shared_panel<T>(st, SharedPanelOp::rhs, a_rhs); }          // LinearSystemSolvers.jl:134-136
        { ProfLaunchScope ps(prof, cat_fwd, lvl); shared_panel<T>(st, SharedPanelOp::forward, a_fwd); }      // :137, L y = t
        { ProfLaunchScope ps(prof, cat_bwd, lvl); shared_panel<T>(st, SharedPanelOp::backward_x, a_bwd); }   // :137, L' x~ = y; SolveQuadraticProgram.jl:56-57
        { ProfLaunchScope ps(prof, cat_pass, lvl); shared_panel<T>(st, op_row, a_row); }                     // :139; SolveQuadraticProgram.jl:59-61
    }
    void check_products(const T* xv, const T* yv) override {
        shared_panel<T>(st, SharedPanelOp::product, product_args(A, NP, MP, NP, xv, Ax));
        shared_panel<T>(st, SharedPanelOp::product, product_args(P, NP, NP, NP, xv, Px));
        shared_panel<T>(st, SharedPanelOp::product, product_args(At, MP, NP, MP, yv, Aty));
    }
};

}  // namespace

int shared_batch_max_np(int dtype) { return 16 * 512 * (dtype == QPS_F64 ? VecOf<double>::N : VecOf<float>::N); }   // whole-factor explicit inverse: 16384 fp64 / 32768 fp32 (k_trsv.hip)

BatchSolverBase* make_dense_shared_batch(int device, int dtype, int count, int64_t n, int64_t m, const double* P, int64_t ldp, const double* A, int64_t lda,
                                         const double* q, const double* l, const double* u) {
    auto load = [&](auto s) { s->load(P, ldp, A, lda, q, l, u); return static_cast<BatchSolverBase*>(s.release()); };   // a unique_ptr: a throw while loading drops the solver
    if (dtype == QPS_F64) return load(std::make_unique<SharedBatchSolver<double>>(device, count, n, m));
    return load(std::make_unique<SharedBatchSolver<float>>(device, count, n, m));
}

}  // namespace qps
