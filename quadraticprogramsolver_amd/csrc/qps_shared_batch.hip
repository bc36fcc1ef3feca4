// qps_shared_batch.hip -- the shared-matrix batches: `count` QPs on ONE P and ONE A that differ in q, l, u only.  One host driver of the ADMM loop
// (SharedFamilySolver: SolveQuadraticProgram.jl:36-73 for every column at once, every option of qps_set_shared_*), three linear-system paths under it: the dense
// Cholesky on MFMA panels (SharedBatchSolver, k_shared.hip), the sparse KKT L D L' with panel sweeps (SparseSharedBatchSolver, k_ldl.hip, k_csr_panel.hip) and
// the matrix-free CG on panels (CgSharedBatchSolver, k_cg_panel.hip).
// qps_capi.hip validates the caller's arrays and builds the handles through the three factories at the end of this file.
#include <limits>
#include <memory>

#include "dense_chol.h"
#include "qps_batch.h"
#include "qps_ldl.h"
#include "qps_polish.h"
#include "shared_family_rules.h"
#include "spmv_layout.h"

namespace qps {
namespace {

// the range check of the equilibration: every non-zero scaled matrix entry has to stay a normal number of the handle's type
template <typename T> inline void equil_check_range(double hi, double lo, const char* fn = "qps_set_shared_equilibration") {
    if (hi > (double)std::numeric_limits<T>::max() || lo < (double)std::numeric_limits<T>::min()) {
        char b[256];
        snprintf(b, sizeof b, "%s: a scaled matrix entry would leave the normal range of the handle's type (largest %.3g, smallest non-zero %.3g, "
                              "range %.3g .. %.3g); the handle is unchanged", fn, hi, lo, (double)std::numeric_limits<T>::min(), (double)std::numeric_limits<T>::max());
        throw QpsError(QPS_ERR_UNSUPPORTED, b);
    }
}
// |(T) v| 2^e of one new matrix entry under a kept exponent, into the running range (qps_update_shared_matrices*: checked on the host before anything is modified)
template <typename T> inline void equil_range_add(double v, int e, double& hi, double& lo) {
    const double a = std::ldexp(std::fabs((double)(T)v), e);
    hi = std::fmax(hi, a);
    if (a > 0) lo = std::fmin(lo, a);
}
// qps_update_shared_matrices_csc: the canonical pattern of a given matrix has to be the handle's, entry for entry (an explicit zero is part of it)
inline void require_same_pattern(const char* name, int64_t ncols, const std::vector<int64_t>& cp, const std::vector<int64_t>& ri, const CanonicalCsc& c) {
    if (!c.given) return;
    for (int64_t j = 0; j < ncols; ++j) {
        const int64_t a0 = cp[(size_t)j], a1 = cp[(size_t)j + 1], b0 = c.cp[(size_t)j], b1 = c.cp[(size_t)j + 1];
        if (a1 - a0 == b1 - b0 && std::equal(ri.begin() + a0, ri.begin() + a1, c.ri.begin() + b0)) continue;
        char b[256];
        snprintf(b, sizeof b, "qps_update_shared_matrices_csc: the sparsity pattern of %s differs from the handle's (first in column %lld, 0-based; %lld stored entries there "
                              "against %lld); the handle is unchanged", name, (long long)j, (long long)(b1 - b0), (long long)(a1 - a0));
        throw QpsError(QPS_ERR_BAD_ARGUMENT, b);
    }
}

// =================================================================================================================
// What the two paths have in common: the resources, the state in 16-column panels [panel][rows][16] (rows = rowsN for n-vectors, rowsM for m-vectors), the
// options, and the loop.  rho is common (a common factor needs a common rho): fixed, or moved for the whole family by qps_set_shared_adaptive_rho; every column
// keeps its own check, flag, stopping iteration and residuals, and a column that stopped is frozen by the active mask, exactly as BatchedDenseSolver does.
// A path supplies its matrices, its factorisation and the hooks at the end of the class; a hook owns every launch of its step, in the path's own order.
// =================================================================================================================
template <typename T> struct SharedFamilySolver : BatchSolverBase, SharedFamilyOps {
    StreamLease lease; DeviceOwner mem; hipStream_t st = nullptr;   // destroyed in reverse: the uploader's events, buffers, then the stream lease, then the Profiler
    std::unique_ptr<StagedUploader> up;   // its pinned double buffer lives as long as the handle: every solve uploads warm starts
    int CP = 0, npanel = 0, rowsN = 0, rowsM = 0;
    T *q = nullptr, *l = nullptr, *u = nullptr, *x = nullptr, *xp = nullptr, *z = nullptr, *zp = nullptr, *y = nullptr, *Ax = nullptr, *Px = nullptr, *Aty = nullptr;
    int* d_active = nullptr; int* h_int = nullptr;
    unsigned long long* slots = nullptr; double* res_dev = nullptr; double* res_host = nullptr; double* stage = nullptr;
    bool factor_valid = false; double fac_rho = 0, fac_sigma = 0; int num_factorizations = 0;
    int cat_chk = 0, cat_fac = 0, cat_switch = 0, cat_start = 0;
    int info_trsv_block = 0, info_sweep_variant = 0;   // what qps_info reports for the path
    // Per-row rho scale (qps_set_shared_rho_scale): row i runs with rho_i = rho s_i; rs_rho / rs_rho1 hold rho_i and 1 / rho_i (rowsM long, padding rows: scale 1),
    // formed in double and rounded once, for the base rho rs_base (0: stale).  The buffers exist only while a scale is set.
    std::vector<double> rho_scale; T *rs_rho = nullptr, *rs_rho1 = nullptr; double rs_base = 0;
    // Equilibration (qps_set_shared_equilibration): while it is on, the path's matrices hold D P D and E A D, q, l, u hold D q, E l, E u -- scaled in place by exact
    // powers of two, undone in place when it is cleared -- and kd / ke (rowsN / rowsM ints) are the exponents on the device; the loop kernels run as they are.
    int *kd = nullptr, *ke = nullptr;
    // Infeasibility certificates (qps_set_shared_infeasibility): while a tolerance is set the handle holds yp (y before the row update of a check iteration), the
    // projected difference dyh (rowsM) and dxp = x - xp (rowsN) as panels, and the partial sums of the reduction; last_conv: the flags of the last solve.
    double inf_epsP = 0, inf_epsD = 0; T *yp = nullptr, *dyh = nullptr, *dxp = nullptr; double* cert_part = nullptr; int cat_inf = 0;
    std::vector<int> last_conv;
    std::vector<int> active;   // the host copy of the mask of the running solve (CP long)

    SharedFamilySolver(int dev, int cnt, int64_t n_, int64_t m_, int rowsN_, int rowsM_) {
        device = dev; n = n_; m = m_; count = cnt;
        HIPC(hipSetDevice(device));
        st = prof.st = lease.acquire(device);
        CP = roundup(count, 16); npanel = CP / 16; rowsN = rowsN_; rowsM = rowsM_;
        up.reset(new StagedUploader(st));
    }
    // The stream idle and no event left on it.  The destructor of a path calls this first: its own members go before this class's destructor body runs.
    void drain() {
        (void)hipSetDevice(device);
        (void)hipStreamSynchronize(st);
        prof.release_events();
    }
    ~SharedFamilySolver() override { drain(); }
    SharedFamilyOps* shared_family() override { return this; }

    void alloc_check_buffers() {   // the mask, the check's slots and read-back, the staging of put_panels / get_panels
        d_active = mem.dalloc<int>(CP, st); h_int = mem.pinned<int>(CP + 4);
        slots = mem.dalloc<unsigned long long>(16 * (int64_t)CP, st); res_dev = mem.dalloc<double>(8 * (int64_t)CP, st); res_host = mem.pinned<double>(8 * (size_t)CP);
        stage = mem.dalloc<double>((int64_t)count * std::max(n, m) + 64, st);
    }
    // a host CSR matrix on the device as the CSR x panel products read it (the sparse paths: the check's P, A, A'; the CG path's operator)
    CsrPanelMatrix<T> upload_csr(const layout::CsrHost& h) {
        CsrPanelMatrix<T> M; M.rows = h.nrows;
        int* rp = mem.dalloc<int>((int64_t)h.rp.size(), st); int* ci = mem.dalloc<int>((int64_t)h.ci.size(), st);
        T* va = mem.dalloc<T>((int64_t)h.va.size(), st);
        std::vector<T> v(h.va.begin(), h.va.end());
        up->copy(rp, h.rp.data(), sizeof(int) * h.rp.size());
        if (!h.ci.empty()) { up->copy(ci, h.ci.data(), sizeof(int) * h.ci.size()); up->copy(va, v.data(), sizeof(T) * v.size()); }
        M.rp = rp; M.ci = ci; M.va = va; M.spr = csr_panel_spr((int64_t)h.ci.size(), h.nrows);
        return M;
    }
    // host [count][len] doubles -> panels (padding rows and columns zero); ordered on the stream, the host array is free when this returns
    void put_panels(const double* h, T* d, int64_t len, int rowsP) {
        HIPC(hipMemsetAsync(d, 0, sizeof(T) * (size_t)CP * rowsP, st));
        up->copy(stage, h, sizeof(double) * (size_t)count * (size_t)len);
        to_panels<T>(st, stage, count, (int)len, rowsP, d);
        HIPC(hipStreamSynchronize(st));
    }
    void get_panels(const T* d, double* h, int64_t len, int rowsP) {
        from_panels<T>(st, d, count, (int)len, rowsP, stage);
        HIPC(hipMemcpyAsync(h, stage, sizeof(double) * (size_t)count * (size_t)len, hipMemcpyDeviceToHost, st));
        HIPC(hipStreamSynchronize(st));
    }
    void update_vectors(const double* qh, const double* lh, const double* uh) override {   // the factor depends on P, A, rho, sigma only: it stays valid
        HIPC(hipSetDevice(device));
        if (qh) { put_panels(qh, q, n, rowsN); if (kd) panel_rowscale<T>(st, q, kd, 1, rowsN, npanel, q); }    // q~ = D q
        if (lh) { put_panels(lh, l, m, rowsM); if (kd) panel_rowscale<T>(st, l, ke, 1, rowsM, npanel, l); }    // l~ = E l, u~ = E u (infinite stays infinite)
        if (uh) { put_panels(uh, u, m, rowsM); if (kd) panel_rowscale<T>(st, u, ke, 1, rowsM, npanel, u); }
    }
    void get_dual(double* zh, double* yh) override {
        HIPC(hipSetDevice(device));
        if (!kd) {
            if (zh) get_panels(z, zh, m, rowsM);
            if (yh) get_panels(y, yh, m, rowsM);
            return;
        }
        // z = E^-1 z~, y = E y~ through the check's scratch panel: the state of the handle stays as the solve left it
        if (zh) { panel_rowscale<T>(st, z, ke, -1, rowsM, npanel, Ax); get_panels(Ax, zh, m, rowsM); }
        if (yh) { panel_rowscale<T>(st, y, ke, 1, rowsM, npanel, Ax); get_panels(Ax, yh, m, rowsM); }
    }
    void set_dual(const double* zh, const double* yh) override {   // the counterpart of get_dual: z~ = E z, y~ = E^-1 y
        HIPC(hipSetDevice(device));
        if (zh) { put_panels(zh, z, m, rowsM); if (kd) panel_rowscale<T>(st, z, ke, 1, rowsM, npanel, z); }
        if (yh) { put_panels(yh, y, m, rowsM); if (kd) panel_rowscale<T>(st, y, ke, -1, rowsM, npanel, y); }
        HIPC(hipStreamSynchronize(st));
    }
    // the vectors the handle keeps between calls, in place: *= 2^(+-k) by the exponents in kd / ke (what both paths' apply_equilibration end with)
    void set_infeasibility(double epsPrimInf, double epsDualInf) override {
        HIPC(hipSetDevice(device));
        HIPC(hipStreamSynchronize(st));
        if (epsPrimInf > 0 || epsDualInf > 0) {
            if (!dyh) dyh = mem.dalloc<T>((int64_t)CP * rowsM, st);
            if (!dxp) dxp = mem.dalloc<T>((int64_t)CP * rowsN, st);
            if (!cert_part) cert_part = mem.dalloc<double>(8 * (int64_t)CP * shared_cert_blocks((int)n, (int)m), st);
            if (!yp) yp = mem.dalloc<T>((int64_t)CP * rowsM, st);
        } else {
            mem.release(yp); mem.release(dyh); mem.release(dxp); mem.release(cert_part);
            yp = dyh = dxp = nullptr; cert_part = nullptr;
        }
        inf_epsP = epsPrimInf; inf_epsD = epsDualInf;
    }
    // row b: dyh (flag 4) or dx (flag 5) of column b's own stopping check in the caller's units (dyh = E dyh~, dx = D dx~ through the check's scratch panels), else zeros
    void get_certificate(double* dyo, double* dxo) override {
        HIPC(hipSetDevice(device));
        auto fetch = [&](double* out, const T* src, const int* k, T* scratch, int64_t len, int rowsP, int flag) {
            if (!out) return;
            if (!src || last_conv.empty()) { std::fill(out, out + (size_t)count * (size_t)len, 0.0); return; }
            if (k) { panel_rowscale<T>(st, src, k, 1, rowsP, npanel, scratch); src = scratch; }
            get_panels(src, out, len, rowsP);
            for (int b = 0; b < count; ++b) if (last_conv[b] != flag) std::fill(out + (size_t)b * len, out + (size_t)(b + 1) * len, 0.0);
        };
        fetch(dyo, dyh, ke, Ax, m, rowsM, QPS_CONV_PRIMAL_INFEASIBLE);
        fetch(dxo, dxp, kd, Px, n, rowsN, QPS_CONV_DUAL_INFEASIBLE);
    }
    void rescale_kept_vectors(int sign) {
        panel_rowscale<T>(st, q, kd, sign, rowsN, npanel, q);
        for (T* v : {l, u, z}) panel_rowscale<T>(st, v, ke, sign, rowsM, npanel, v);
        panel_rowscale<T>(st, y, ke, -sign, rowsM, npanel, y);
    }
    void push_row_rho(double rho) {   // rho_i and 1 / rho_i for this base rho
        if (rs_base == rho) return;
        std::vector<T> h((size_t)rowsM), h1((size_t)rowsM);
        for (int i = 0; i < rowsM; ++i) { const double r = rho * (i < m ? rho_scale[i] : 1.0); h[i] = (T)r; h1[i] = (T)(1.0 / r); }
        up->copy(rs_rho, h.data(), sizeof(T) * (size_t)rowsM);
        up->copy(rs_rho1, h1.data(), sizeof(T) * (size_t)rowsM);
        HIPC(hipStreamSynchronize(st));
        rs_base = rho;
    }
    void push_active() {
        for (int b = 0; b < CP; ++b) h_int[b] = active[b];
        HIPC(hipMemcpyAsync(d_active, h_int, sizeof(int) * CP, hipMemcpyHostToDevice, st));
        HIPC(hipStreamSynchronize(st));   // the pinned staging is reused
    }

    void solve_batch(double* xh, const qps_params& p, qps_info* infos) override {
        HIPC(hipSetDevice(device));
        check_params(p);
        const double t0 = now_s();
        if (family_rho && !(p.fctrRho > 0)) throw QpsError(QPS_ERR_BAD_ARGUMENT, "fctrRho must be positive");
        double rho = p.rho, rhorho = rho;                                                           // :43; rho moves under the family rule only
        const double sigma = p.sigma, alpha = p.alpha;
        const double epsAdmm = std::fmin(p.epsAbs, p.epsRel) * 1e-2;                                // SolveQuadraticProgram.jl:34
        const bool reuse = p.reuseFactor && factor_valid && fac_rho == rho && fac_sigma == sigma;
        if (!rho_scale.empty()) push_row_rho(rho);
        if (!reuse) { ProfScope ps(prof, cat_fac, 1); factor_at_setup(rho, sigma, p); }             // :36, once for all columns
        put_panels(xh, x, n, rowsN);
        if (kd) panel_rowscale<T>(st, x, kd, -1, rowsN, npanel, x);                                 // warm start in the scaled variables: x~ = D^-1 x
        active.assign(CP, 0);
        for (int b = 0; b < count; ++b) active[b] = 1;
        const bool certify = inf_epsP > 0 || inf_epsD > 0;                                          // qps_set_shared_infeasibility
        last_conv.clear();
        if (certify) {
            HIPC(hipMemsetAsync(dyh, 0, sizeof(T) * (size_t)CP * rowsM, st));
            HIPC(hipMemsetAsync(dxp, 0, sizeof(T) * (size_t)CP * rowsN, st));
        }
        begin_solve(warm_start, rho, sigma, alpha);                                                 // :38-41
        std::vector<int> conv(count, QPS_CONV_NUM_ITR), iters(count, p.numIterations);
        std::vector<double> resP(count, NAN), resD(count, NAN);
        const double t1 = now_s();
        int nactive = count;
        std::vector<int> nref(count, 0); std::vector<double> rho_col(count, rho), prop_col(count, rho); double tref = 0;
        for (int ii = 1; ii <= p.numIterations && nactive > 0; ++ii) {                              // :45
            if (family_rho && ((rhorho * p.fctrRho < rho) || (rhorho > p.fctrRho * rho))) {         // :47, once for the family
                const double ta = now_s();
                {
                    ProfScope ps(prof, cat_switch, 1);
                    rho = rhorho;
                    switch_rho(rho, sigma);
                }
                for (int b = 0; b < count; ++b) if (active[b]) { ++nref[b]; rho_col[b] = rho; }
                HIPC(hipStreamSynchronize(st));                                                     // tRefactor: host wall time until the device has finished the switch
                tref += now_s() - ta;
            }
            const int lvl = (prof.level == 1 && ii % 50 == 13) ? 1 : 2;   // level 1: one sample of each category in 50 iterations
            const bool at_check = ii % p.numItrConv == 0;
            if (certify && at_check) HIPC(hipMemcpyAsync(yp, y, sizeof(T) * (size_t)CP * rowsM, hipMemcpyDeviceToDevice, st));   // y before this iteration's row update
            iterate(lvl, rho, sigma, alpha);                                                        // LinearSystemSolvers.jl, SolveQuadraticProgram.jl:56-61
            if (!at_check) continue;                                                                // :63
            {
                ProfScope ps(prof, cat_chk, 2);
                HIPC(hipMemsetAsync(slots, 0, 16 * sizeof(unsigned long long) * (size_t)CP, st));
                check_products(x, y);                                                               // mA * vX, mP * vX, mA' * vY
                shared_check<T>(st, (int)n, (int)m, rowsN, rowsM, npanel, Ax, Px, Aty, q, x, xp, z, zp, slots, res_dev, d_active, p.epsAbs, p.epsRel, epsAdmm, rho, kd, ke);   // :64
            }
            if (certify) {   // OSQP 3.4 on the columns the check left running: the check is done with Ax, Px, Aty, which now take A dx, P dx, A'dyh
                ProfScope ps(prof, cat_inf, 2);
                shared_deltas<T>(st, (int)n, (int)m, rowsN, rowsM, npanel, x, xp, y, yp, l, u, d_active, dxp, dyh);
                check_products(dxp, dyh);
                shared_certificates<T>(st, (int)n, (int)m, rowsN, rowsM, npanel, dxp, dyh, Ax, Px, Aty, q, l, u, d_active, kd, ke, cert_part, res_dev, inf_epsP, inf_epsD);
            }
            HIPC(hipMemcpyAsync(res_host, res_dev, 8 * sizeof(double) * (size_t)CP, hipMemcpyDeviceToHost, st));
            HIPC(hipStreamSynchronize(st));
            prof.harvest();
            bool any_done = false;
            for (int b = 0; b < count; ++b) {
                if (!active[b]) continue;
                const double* r = res_host + 8 * b;
                resP[b] = r[0]; resD[b] = r[1]; conv[b] = (int)r[5];
                if (conv[b] != QPS_CONV_NUM_ITR) { active[b] = 0; iters[b] = ii; --nactive; any_done = true; }   // :66-68: x, z, y of this column are frozen from here on
            }
            if (family_rho) {
                rhorho = family_rho_proposal(res_host, active, count, rho, rhorho);
                for (int b = 0; b < count; ++b) if (active[b] || iters[b] == ii) prop_col[b] = rhorho;
            }
            if (any_done && nactive > 0) push_active();
        }
        HIPC(hipStreamSynchronize(st));
        prof.harvest();
        const double t2 = now_s();
        std::vector<PolishReport> pol; double tpol = 0;
        if (polish_on) {                                                                            // qps_set_shared_polish: the step on this solve's own x and y
            std::vector<int> take(count);
            for (int b = 0; b < count; ++b) take[b] = conv[b] != QPS_CONV_PRIMAL_INFEASIBLE && conv[b] != QPS_CONV_DUAL_INFEASIBLE;
            polish_panels(y, x, p, take, pol);
            tpol = now_s() - t2;
        }
        if (kd) { panel_rowscale<T>(st, x, kd, 1, rowsN, npanel, Px); get_panels(Px, xh, n, rowsN); }   // x = D x~ (through the check's scratch panel)
        else get_panels(x, xh, n, rowsN);
        last_conv = conv;
        for (int b = 0; b < count && infos; ++b) {
            qps_info& in = infos[b];
            in.convFlag = conv[b]; in.iterations = iters[b]; in.numRefactor = nref[b]; in.cgIterations = (int)column_cg_iterations(b);
            in.rhoFinal = rho_col[b]; in.rhoProposed = prop_col[b]; in.resPrim = resP[b]; in.resDual = resD[b];
            in.tSetup = t1 - t0; in.tLoop = t2 - t1; in.tRefactor = tref;   // wall time of the whole batch
            in.polishFlag = -1; in.polishIterations = 0; in.tPolish = tpol;
            if (polish_on) { in.polishFlag = pol[b].flag; in.polishIterations = pol[b].minresIterations; }
            in.trsvBlock = info_trsv_block; in.sweepVariant = info_sweep_variant; in.sweepGaveUp = 0; in.cgExplicit = 0;
        }
    }

    // qps_polish_shared: the step from the caller's x and y (NULL: the y the handle holds), in work panels of this call; nothing the handle keeps is written
    void polish(double* xh, const double* yh, const qps_params& p, qps_polish_report* reports) override {
        HIPC(hipSetDevice(device));
        DeviceOwner wm;
        T* xb = wm.dalloc<T>((int64_t)CP * rowsN, st); T* yb = yh ? wm.dalloc<T>((int64_t)CP * rowsM, st) : nullptr;
        put_panels(xh, xb, n, rowsN);
        if (kd) panel_rowscale<T>(st, xb, kd, -1, rowsN, npanel, xb);                               // x~ = D^-1 x
        if (yh) { put_panels(yh, yb, m, rowsM); if (kd) panel_rowscale<T>(st, yb, ke, -1, rowsM, npanel, yb); }   // y~ = E^-1 y
        std::vector<PolishReport> pol;
        polish_panels(yh ? yb : y, xb, p, std::vector<int>(), pol);
        if (kd) panel_rowscale<T>(st, xb, kd, 1, rowsN, npanel, xb);                                // x = D t~_x
        std::vector<double> xo((size_t)count * (size_t)n);
        get_panels(xb, xo.data(), n, rowsN);
        for (int b = 0; b < count; ++b) {
            if (pol[b].flag == 0) std::copy(xo.begin() + (size_t)b * n, xo.begin() + (size_t)(b + 1) * n, xh + (size_t)b * n);   // :322-325; other columns keep every bit
            if (!reports) continue;
            qps_polish_report& r = reports[b];
            r.flag = pol[b].flag; r.refinements = pol[b].refinements; r.minresIterations = pol[b].minresIterations; r.numActiveLower = pol[b].numLower;
            r.numActiveUpper = pol[b].numUpper; r.reserved0 = 0; r.relres = pol[b].relres; r.seconds = pol[b].seconds;
        }
    }
    // SolveQuadraticProgram.m:289-325 for the columns of `take` (empty: all), all at once, on the data the handle holds (the scaled data while the equilibration
    // is on): ypan are rowsM panels, xpan rowsN panels that take t_x where the column's last MINRES call converged.  K v comes from check_products -- the
    // matrices are read once per MINRES iteration for all columns of a panel pair -- and k_shared_polish.hip does the rest.  The columns advance in lockstep:
    // in round jj those still refining form g - K t and run MINRES together, the host reading the per-column states every 8 iterations; a column whose call
    // ended with flag 1 leaves with its x kept (:316-318), the others add tt and go on.  The work panels live for this call only.
    void polish_panels(const T* ypan, T* xpan, const qps_params& p, const std::vector<int>& take, std::vector<PolishReport>& reps) {
        const double t0 = now_s();
        reps.assign(count, PolishReport());
        if (p.numItrPolish <= 0) return;                                                            // :292
        SharedPolishGeom g; g.n = (int)n; g.m = (int)m; g.rowsN = rowsN; g.rowsM = rowsM; g.npanel = npanel;
        const int64_t N = (int64_t)CP * (rowsN + rowsM), ML = (int64_t)CP * rowsM; const int nblk = shared_polish_blocks(rowsN, rowsM);
        DeviceOwner wm;
        T* gv = wm.dalloc<T>(9 * N + 2 * ML, st);
        T *t = gv + N, *tt = t + N, *rhs = tt + N, *c = rhs + N, *r1 = c + N, *r2 = r1 + N, *w1 = r2 + N, *w2 = w1 + N, *mask = w2 + N, *wl = mask + ML;   // t = tt = 0 (:307-308)
        double* pa = wm.dalloc<double>(2 * (int64_t)CP * nblk, st); double* pb = pa + (int64_t)CP * nblk;
        SharedPolishState* state = wm.dalloc<SharedPolishState>(2 * (int64_t)CP, st);
        int* counts = wm.dalloc<int>(3 * (int64_t)CP, st); int* live_dev = counts + 2 * CP;
        SharedPolishState* hs = wm.pinned<SharedPolishState>((size_t)CP); int* hi = wm.pinned<int>(3 * (size_t)CP);
        std::vector<int> live(CP, 0);
        int nlive = 0;
        for (int b = 0; b < count; ++b) nlive += live[b] = take.empty() || take[b];
        auto push_live = [&] {
            for (int b = 0; b < CP; ++b) hi[2 * CP + b] = live[b];
            HIPC(hipMemcpyAsync(live_dev, hi + 2 * CP, sizeof(int) * CP, hipMemcpyHostToDevice, st));
            HIPC(hipStreamSynchronize(st));
        };
        shared_polish_setup<T>(st, g, q, l, u, ypan, mask, gv, counts);                             // :293-299
        HIPC(hipMemcpyAsync(hi, counts, sizeof(int) * 2 * CP, hipMemcpyDeviceToHost, st));
        push_live();
        const SharedPolishProducts<T> k{mask, wl, Ax, Px, Aty};
        const T delta = (T)p.delta;
        for (int jj = 0; jj < p.numItrPolish && nlive > 0; ++jj) {                                  // :314
            shared_polish_wl<T>(st, g, mask, t, wl);
            check_products(t, wl);
            shared_polish_rhs<T>(st, g, live_dev, gv, t, k, rhs);                                   // g - K t
            shared_polish_wl<T>(st, g, mask, tt, wl);
            check_products(tt, wl);                                                                 // KK x0, x0 = the tt of the previous round
            shared_polish_begin<T>(st, g, live_dev, delta, rhs, tt, k, r1, r2, w1, w2, pa, pb, state, p.epsMinres, p.numItrMinres);   // :315
            shared_polish_wl<T>(st, g, mask, r2, wl);
            int cur = 0, launched = 0;
            auto any_running = [&] {
                HIPC(hipMemcpyAsync(hs, state + (int64_t)cur * CP, sizeof(SharedPolishState) * (size_t)CP, hipMemcpyDeviceToHost, st));
                HIPC(hipStreamSynchronize(st));
                for (int b = 0; b < count; ++b) if (live[b] && !hs[b].done) return true;
                return false;
            };
            bool running = any_running();
            while (running && launched < p.numItrMinres) {
                for (int burst = std::min(8, p.numItrMinres - launched); burst > 0; --burst) {
                    check_products(r2, wl);                                                         // KK y (= beta KK v)
                    shared_polish_step<T>(st, g, state + (int64_t)cur * CP, state + (int64_t)(cur ^ 1) * CP, delta, k, c, r1, r2, w1, w2, tt, pa, pb);
                    std::swap(r1, r2); std::swap(w1, w2);                                           // r2 = the new Lanczos vector, w2 = the new w
                    cur ^= 1; ++launched;
                }
                running = any_running();
            }
            for (int b = 0; b < count; ++b) {
                if (!live[b]) continue;
                const SharedPolishState& s = hs[b];
                PolishReport& r = reps[b];
                r.flag = s.done ? s.flag : 1; r.minresIterations += s.itn; r.refinements = jj + 1; r.relres = s.bnorm == 0.0 ? 0.0 : s.phibar / s.bnorm;
                if (r.flag) { live[b] = 0; --nlive; }                                               // :316-318
            }
            push_live();
            if (nlive > 0) shared_polish_add<T>(st, g, live_dev, state + (int64_t)cur * CP, t, tt); // :319
        }
        for (int b = 0; b < count; ++b) live[b] = reps[b].flag == 0;
        push_live();
        shared_polish_select<T>(st, g, live_dev, t, xpan);                                          // :322-325
        HIPC(hipStreamSynchronize(st));
        const double secs = now_s() - t0;
        for (int b = 0; b < count; ++b) { reps[b].numLower = hi[2 * b]; reps[b].numUpper = hi[2 * b + 1]; reps[b].seconds = secs; }
    }

  protected:
    virtual void check_params(const qps_params& p) = 0;                               // the path's refusals
    virtual void factor_at_setup(double rho, double sigma, const qps_params& p) = 0;  // no reusable factor: LinSysSolInit for (rho, sigma)
    // Zero the start state for warm start mode `warm` (the path's panels included), call push_active(), run the mode 1 / 2 start launches under cat_start and
    // prepare the launch arguments of this solve.
    virtual void begin_solve(int warm, double rho, double sigma, double alpha) = 0;
    virtual void switch_rho(double rho, double sigma) = 0;                            // the family moved to `rho`: new factor, state that held the previous rho
    virtual void iterate(int lvl, double rho, double sigma, double alpha) = 0;        // one ADMM iteration of every active column, profiled at level `lvl`
    // Ax = A xv, Px = P xv, Aty = A'yv for arbitrary panels (the check's x, y; the certificates' dx, dyh; the polishing step's v_x, mask v_lambda); usable outside a solve
    virtual void check_products(const T* xv, const T* yv) = 0;
    virtual int64_t column_cg_iterations(int) { return 0; }                           // qps_info.cgIterations of column b of the running solve (a path without CG: 0)
};

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
    using B::cat_chk; using B::cat_fac; using B::cat_switch; using B::cat_start; using B::rho_scale; using B::rs_rho; using B::rs_rho1; using B::rs_base;
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
        q = mem.template dalloc<T>(pn, st); x = mem.template dalloc<T>(pn, st); xp = mem.template dalloc<T>(pn, st); xx = mem.template dalloc<T>(pn, st);
        tt = mem.template dalloc<T>(pn, st); yv = mem.template dalloc<T>(pn, st); Px = mem.template dalloc<T>(pn, st); Aty = mem.template dalloc<T>(pn, st);
        l = mem.template dalloc<T>(pm, st); u = mem.template dalloc<T>(pm, st); z = mem.template dalloc<T>(pm, st); zp = mem.template dalloc<T>(pm, st);
        y = mem.template dalloc<T>(pm, st); w = mem.template dalloc<T>(pm, st); Ax = mem.template dalloc<T>(pm, st);
        for (T* v : {z, y}) HIPC(hipMemsetAsync(v, 0, sizeof(T) * (size_t)pm, st));                 // the state qps_set_shared_warm_start continues from is defined from creation on
        fail = mem.template dalloc<int>(4, st);
        this->alloc_check_buffers();
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
    void set_rho_scale(const double* s) override {
        HIPC(hipSetDevice(device));
        HIPC(hipStreamSynchronize(st));
        if (!s) {
            for (T** v : {&Ws, &rs_sqrt, &rs_rho, &rs_rho1}) { mem.release(*v); *v = nullptr; }
            rho_scale.clear();
        } else {
            if (!Ws) Ws = mem.template dalloc<T>((int64_t)MP * NP, st);
            if (!rs_sqrt) rs_sqrt = mem.template dalloc<T>(MP, st);
            if (!rs_rho) rs_rho = mem.template dalloc<T>(MP, st);
            if (!rs_rho1) rs_rho1 = mem.template dalloc<T>(MP, st);
            std::vector<T> h((size_t)MP, T(1));
            for (int64_t i = 0; i < m; ++i) h[i] = (T)std::sqrt(s[i]);
            up->copy(rs_sqrt, h.data(), sizeof(T) * (size_t)MP);
            scale_rows<T>(st, A, rs_sqrt, MP, NP, Ws);
            HIPC(hipStreamSynchronize(st));
            rho_scale.assign(s, s + m);
        }
        factor_valid = false; have_AA = false; rs_base = 0;   // the cached product and the factor belong to the previous scale
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
        for (T* v : {xp, xx, tt, yv}) HIPC(hipMemsetAsync(v, 0, sizeof(T) * (size_t)CP * NP, st));  // :38
        if (warm == 0) { for (T* v : {z, zp, y, w}) HIPC(hipMemsetAsync(v, 0, sizeof(T) * (size_t)CP * MP, st)); }   // :39-41
        else { for (T* v : {zp, w}) HIPC(hipMemsetAsync(v, 0, sizeof(T) * (size_t)CP * MP, st)); }  // z (mode 1) and y stay: iteration 1 overwrites zp before a check reads it
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

// =================================================================================================================
// Sparse path (a lasso / SVM regularisation path, a scenario sweep on a sparse model).  The linear system is the sparse L D L' of the KKT matrix (k_ldl.hip):
// ordering and symbolic factor once at creation (host only), ONE numeric factorisation per (rho, sigma), and every iteration runs the level-scheduled sweeps on
// 16-column panels -- the index and value of a factor entry are loaded once for 16 QPs, the launch chain is paid once per batch.  The check's A x, P x, A'y are
// CSR x panel products (k_csr_panel.hip).  Panels are n and m rows long, without padding rows.
// =================================================================================================================
template <typename T> struct SparseSharedBatchSolver final : SharedFamilySolver<T> {
    using B = SharedFamilySolver<T>;
    using B::device; using B::n; using B::m; using B::prof; using B::mem; using B::st; using B::up; using B::CP; using B::npanel;
    using B::q; using B::l; using B::u; using B::x; using B::xp; using B::z; using B::zp; using B::y; using B::Ax; using B::Px; using B::Aty;
    using B::d_active; using B::factor_valid; using B::fac_rho; using B::fac_sigma; using B::num_factorizations;
    using B::cat_chk; using B::cat_fac; using B::cat_switch; using B::cat_start; using B::rho_scale; using B::rs_rho; using B::rs_rho1; using B::rs_base;
    using B::kd; using B::ke; using B::eq_kd; using B::eq_ke; using B::upload_csr;
    std::unique_ptr<SparseLdl<T>> ldl;   // reads rs_rho / rs_rho1 in its numeric factorisation and panel kernels while a scale is set
    CsrPanelMatrix<T> P, A, At;
    LdlPanelProf pf;
    // Equilibration: the exponents come from the host copy of the canonical CSC arrays (values rounded to T); while it is on, the factor's value array and the
    // three CSR value arrays of the check hold the scaled entries.  Ordering, symbolic factor and every index array stay as they are.
    std::vector<int64_t> hPcp, hPri, hAcp, hAri; std::vector<double> hPnz, hAnz;
    // qps_update_shared_matrices_csc, from its first call on: the staging of the canonical values (nnz(P) + nnz(A) doubles), the position of every entry of the
    // by-rows copy of A in CSC order, and -- while the equilibration is on -- the exponent of every entry of the four value arrays
    double* upd_src = nullptr; int *upd_map = nullptr, *upd_e = nullptr;
    LdlPanelState<T> s; bool rhs_ready = false;   // the running solve

    SparseSharedBatchSolver(int dev, int cnt, int64_t n_, int64_t m_, SparseSharedInput&& in, const double* qh, const double* lh, const double* uh)
        : B(dev, cnt, n_, m_, (int)n_, (int)m_) {
        layout::CsrHost Ph, Ah, Ath;
        try {
            Ph = layout::csc_as_transposed_csr(n, n, in.Pcp, in.Pri, in.Pnz);      // P: CSC == CSR (symmetric, full storage)
            layout::csc_to_csr_pair(m, n, in.Acp, in.Ari, in.Anz, Ah, Ath);        // rows of A by a counting sort; rows of A' are the columns of A
        } catch (const std::length_error& ex) { throw QpsError(QPS_ERR_BAD_DIMENSION, ex.what()); }
        P = upload_csr(Ph); A = upload_csr(Ah); At = upload_csr(Ath);
        const int64_t pnnz = (int64_t)in.Pnz.size(), annz = (int64_t)in.Anz.size();
        const int64_t nnzL = (int64_t)in.sym.ci.size(); const int N = in.sym.N, Ns = in.sym.Ns, ldt = in.sym.ldt;
        ldl = make_sparse_ldl<T>(st, std::move(in.sym), in.Pnz.data(), pnnz, in.Anz.data(), annz);
        ldl->panels_prepare(npanel, in.spr);
        hPcp = std::move(in.Pcp); hPri = std::move(in.Pri); hPnz = std::move(in.Pnz); hAcp = std::move(in.Acp); hAri = std::move(in.Ari); hAnz = std::move(in.Anz);
        const int64_t pn = (int64_t)CP * n, pm = (int64_t)CP * m;
        q = mem.template dalloc<T>(pn, st); x = mem.template dalloc<T>(pn, st); xp = mem.template dalloc<T>(pn, st); Px = mem.template dalloc<T>(pn, st);
        Aty = mem.template dalloc<T>(pn, st);
        l = mem.template dalloc<T>(pm, st); u = mem.template dalloc<T>(pm, st); z = mem.template dalloc<T>(pm, st); zp = mem.template dalloc<T>(pm, st);
        y = mem.template dalloc<T>(pm, st); Ax = mem.template dalloc<T>(pm, st);
        for (T* v : {z, y}) HIPC(hipMemsetAsync(v, 0, sizeof(T) * (size_t)pm, st));                 // the state qps_set_shared_warm_start continues from is defined from creation on
        this->alloc_check_buffers();
        // algorithmic bytes per iteration (check: per check), counted as SparseLdl::bytes_per_solve does: every factor entry's index and value once per panel,
        // the lines it gathers and the vectors read and written once per column
        const double sz = sizeof(T), c = CP, np = npanel, Nd = N, ents = (double)nnzL;
        pf.prof = &prof;
        pf.cat_rhs = prof.category("sparse shared: rhs (panels)", 4.0 * Nd * np + sz * c * (2.0 * n + 2.0 * m + Nd));
        pf.cat_fwd = prof.category("sparse shared: forward levels (panels)", np * ents * (sz + 4) + sz * c * (ents + 2.0 * Nd));
        pf.cat_tail = prof.category("sparse shared: dense tail (MFMA panels)", sz * ((double)ldt * (ldt + 1) + 6.0 * c * ldt));
        pf.cat_bwd = prof.category("sparse shared: backward levels (panels)", np * ents * (sz + 4) + sz * c * (ents + 3.0 * Ns));
        pf.cat_post = prof.category("sparse shared: post + update (panels)", 4.0 * Nd * np + sz * c * (2.0 * Nd + 5.0 * n + 8.0 * m));
        cat_chk = prof.category("sparse shared: check (A x, P x, A'y, norms)", np * (2.0 * annz + pnnz) * (sz + 4) + sz * c * ((2.0 * annz + pnnz) + 8.0 * n + 6.0 * m));
        this->cat_inf = prof.category("sparse shared: infeasibility (deltas, 3 products, sums)",
                                      np * (2.0 * annz + pnnz) * (sz + 4) + sz * c * ((2.0 * annz + pnnz) + 10.0 * n + 10.0 * m));
        cat_fac = prof.category("sparse shared: factorisation at setup", (sz + 4) * ents + sz * (pnnz + annz));
        cat_switch = prof.category("sparse shared: rho switch (numeric L D L')", (sz + 4) * ents + sz * (pnnz + annz));
        cat_start = prof.category("sparse shared: warm start (A x -> z)", np * annz * (sz + 4) + sz * c * (annz + m));
        this->update_vectors(qh, lh, uh);
    }
    ~SparseSharedBatchSolver() override { this->drain(); }   // before ldl and its device buffers go
    bool takes_csc() const override { return true; }
    void update_matrices(const double*, int64_t, const double*, int64_t) override {
        throw QpsError(QPS_ERR_UNSUPPORTED, "qps_update_shared_matrices: a sparse shared-matrix batch takes its matrices through qps_update_shared_matrices_csc");
    }
    // New values on the frozen pattern: one upload of the canonical values as doubles, then one launch per value array (the CSR copies P, A, A' and the factor's
    // [P; A]) that rounds, permutes and scales.  upd_src, upd_map and upd_e are built at the first update and kept; upd_e goes whenever the scaling changes.
    void update_matrices_csc(const CanonicalCsc& Pc, const CanonicalCsc& Ac) override {
        if (!Pc.given && !Ac.given) return;
        HIPC(hipSetDevice(device));
        HIPC(hipStreamSynchronize(st));
        require_same_pattern("P", n, hPcp, hPri, Pc);
        require_same_pattern("A", n, hAcp, hAri, Ac);
        const int64_t pnnz = (int64_t)hPnz.size(), annz = (int64_t)hAnz.size();
        if (kd) {                                                  // the kept exponents on the new values, before anything is modified
            double hi = 0, lo = INFINITY;
            for (int64_t j = 0; j < n; ++j) {
                for (int64_t k = hPcp[j]; Pc.given && k < hPcp[j + 1]; ++k) equil_range_add<T>(Pc.nz[k], eq_kd[hPri[k]] + eq_kd[j], hi, lo);
                for (int64_t k = hAcp[j]; Ac.given && k < hAcp[j + 1]; ++k) equil_range_add<T>(Ac.nz[k], eq_ke[hAri[k]] + eq_kd[j], hi, lo);
            }
            equil_check_range<T>(hi, lo, "qps_update_shared_matrices_csc");
        }
        if (!upd_src) upd_src = mem.template dalloc<double>(pnnz + annz, st);
        if (!upd_map) {
            const std::vector<int> map = layout::csc_rows_position_map(m, n, hAcp, hAri);
            upd_map = mem.template dalloc<int>(annz, st);
            if (annz > 0) up->copy(upd_map, map.data(), sizeof(int) * (size_t)annz);
        }
        if (kd && !upd_e) {
            const std::vector<int> e = entry_exponents(eq_kd, eq_ke);
            upd_e = mem.template dalloc<int>((int64_t)e.size(), st);
            if (!e.empty()) up->copy(upd_e, e.data(), sizeof(int) * e.size());
        }
        const int *eK = upd_e, *eP = upd_e ? upd_e + pnnz + annz : nullptr, *eA = upd_e ? eP + pnnz : nullptr, *eAt = upd_e ? eA + annz : nullptr;
        if (Pc.given && pnnz > 0) {
            up->copy(upd_src, Pc.nz.data(), sizeof(double) * (size_t)pnnz);
            refresh_values<T>(st, upd_src, nullptr, eP, pnnz, const_cast<T*>(P.va));
            ldl->set_values(upd_src, eK, 0, pnnz);
        }
        if (Ac.given && annz > 0) {
            up->copy(upd_src + pnnz, Ac.nz.data(), sizeof(double) * (size_t)annz);
            refresh_values<T>(st, upd_src + pnnz, upd_map, eA, annz, const_cast<T*>(A.va));
            refresh_values<T>(st, upd_src + pnnz, nullptr, eAt, annz, const_cast<T*>(At.va));
            ldl->set_values(upd_src + pnnz, eK ? eK + pnnz : nullptr, pnnz, annz);
        }
        HIPC(hipStreamSynchronize(st));
        if (Pc.given) hPnz = Pc.nz;                                // what a later qps_set_shared_equilibration computes its exponents from
        if (Ac.given) hAnz = Ac.nz;
        factor_valid = false;                                      // the next solve runs the numeric factorisation on the frozen pattern, also with reuseFactor
        this->last_conv.clear();
    }
    // one exponent per entry, in the order of each value array: the factor's [P; A] in CSC order, then the CSR copies P, A, A'
    std::vector<int> entry_exponents(const std::vector<int>& hd, const std::vector<int>& he) const {
        const int64_t pnnz = (int64_t)hPnz.size(), annz = (int64_t)hAnz.size();
        layout::CsrHost Ph = layout::csc_as_transposed_csr(n, n, hPcp, hPri, hPnz), Ah, Ath;
        layout::csc_to_csr_pair(m, n, hAcp, hAri, hAnz, Ah, Ath);
        std::vector<int> e((size_t)(2 * pnnz + 3 * annz));
        int* eK = e.data(); int *eP = eK + pnnz + annz, *eA = eP + pnnz, *eAt = eA + annz;
        for (int64_t j = 0; j < n; ++j) {
            for (int64_t k = hPcp[j]; k < hPcp[j + 1]; ++k) eK[k] = hd[hPri[k]] + hd[j];
            for (int64_t k = hAcp[j]; k < hAcp[j + 1]; ++k) eK[pnnz + k] = he[hAri[k]] + hd[j];
        }
        for (int r = 0; r < Ph.nrows; ++r) for (int k = Ph.rp[r]; k < Ph.rp[r + 1]; ++k) eP[k] = hd[r] + hd[Ph.ci[k]];
        for (int r = 0; r < Ah.nrows; ++r) for (int k = Ah.rp[r]; k < Ah.rp[r + 1]; ++k) eA[k] = he[r] + hd[Ah.ci[k]];
        for (int r = 0; r < Ath.nrows; ++r) for (int k = Ath.rp[r]; k < Ath.rp[r + 1]; ++k) eAt[k] = hd[r] + he[Ath.ci[k]];
        return e;
    }
    // every value array, in place: *= 2^(+-k) by the host exponents hd / he (the vectors the handle keeps are not touched)
    void scale_matrix_values(int sign, const std::vector<int>& hd, const std::vector<int>& he) {
        const int64_t pnnz = (int64_t)hPnz.size(), annz = (int64_t)hAnz.size();
        const std::vector<int> e = entry_exponents(hd, he);
        int* de = mem.template dalloc<int>((int64_t)e.size(), st);
        if (!e.empty()) up->copy(de, e.data(), sizeof(int) * e.size());
        ldl->rescale_values(de, sign);
        scale_entries<T>(st, const_cast<T*>(P.va), de + pnnz + annz, sign, pnnz);
        scale_entries<T>(st, const_cast<T*>(A.va), de + 2 * pnnz + annz, sign, annz);
        scale_entries<T>(st, const_cast<T*>(At.va), de + 2 * pnnz + 2 * annz, sign, annz);
        HIPC(hipStreamSynchronize(st));
        mem.release(de);
    }
    // every value array and every vector the handle keeps between calls, in place (device copies of the exponents in kd / ke)
    void apply_equilibration(int sign, const std::vector<int>& hd, const std::vector<int>& he) {
        this->rescale_kept_vectors(sign);
        scale_matrix_values(sign, hd, he);
    }
    void set_equilibration(int passes) override {
        HIPC(hipSetDevice(device));
        HIPC(hipStreamSynchronize(st));
        // the rule of the dense handle on the host: norms in double from the values rounded to T, read through the exponents
        std::vector<int> hd, he;
        if (passes > 0) {
            const int64_t pnnz = (int64_t)hPnz.size(), annz = (int64_t)hAnz.size();
            std::vector<double> aP((size_t)pnnz), aA((size_t)annz), cn((size_t)n), rn((size_t)m);
            for (int64_t k = 0; k < pnnz; ++k) aP[k] = std::fabs((double)(T)hPnz[k]);
            for (int64_t k = 0; k < annz; ++k) aA[k] = std::fabs((double)(T)hAnz[k]);
            hd.assign((size_t)n, 0); he.assign((size_t)m, 0);
            double hi = 0, lo = INFINITY;
            for (int pass = 0; pass <= passes; ++pass) {           // the last round only measures the range of the scaled entries
                std::fill(cn.begin(), cn.end(), 0.0); std::fill(rn.begin(), rn.end(), 0.0);
                hi = 0; lo = INFINITY;
                for (int64_t j = 0; j < n; ++j) {
                    for (int64_t k = hPcp[j]; k < hPcp[j + 1]; ++k) {
                        const double v = std::ldexp(aP[k], hd[hPri[k]] + hd[j]);
                        cn[j] = std::fmax(cn[j], v); hi = std::fmax(hi, v); if (v > 0) lo = std::fmin(lo, v);
                    }
                    for (int64_t k = hAcp[j]; k < hAcp[j + 1]; ++k) {
                        const int64_t i = hAri[k];
                        const double v = std::ldexp(aA[k], he[i] + hd[j]);
                        cn[j] = std::fmax(cn[j], v); rn[i] = std::fmax(rn[i], v); hi = std::fmax(hi, v); if (v > 0) lo = std::fmin(lo, v);
                    }
                }
                if (pass == passes) break;
                for (int64_t j = 0; j < n; ++j) hd[j] = std::max(-EQUIL_CLAMP, std::min(EQUIL_CLAMP, hd[j] + equil_step(cn[j])));
                for (int64_t i = 0; i < m; ++i) he[i] = std::max(-EQUIL_CLAMP, std::min(EQUIL_CLAMP, he[i] + equil_step(rn[i])));
            }
            equil_check_range<T>(hi, lo);                          // before anything is modified
        }
        if (kd) apply_equilibration(-1, eq_kd, eq_ke);             // the caller's values again, bit for bit
        mem.release(kd); mem.release(ke); kd = ke = nullptr;
        mem.release(upd_e); upd_e = nullptr;                       // the per-entry exponents of qps_update_shared_matrices_csc belong to the previous scaling
        eq_kd = hd; eq_ke = he;
        if (passes > 0) {
            kd = mem.template dalloc<int>(n, st); ke = mem.template dalloc<int>(m, st);
            up->copy(kd, hd.data(), sizeof(int) * (size_t)n);
            up->copy(ke, he.data(), sizeof(int) * (size_t)m);
            apply_equilibration(1, hd, he);
        }
        factor_valid = false;                                      // the numeric factor belongs to the previous values
        this->last_conv.clear();                                   // and a certificate to the scaling it was taken in
    }
    void set_rho_scale(const double* sc) override {
        HIPC(hipSetDevice(device));
        HIPC(hipStreamSynchronize(st));
        if (!sc) {
            ldl->set_row_rho(nullptr, nullptr);
            for (T** v : {&rs_rho, &rs_rho1}) { mem.release(*v); *v = nullptr; }
            rho_scale.clear();
        } else {
            if (!rs_rho) rs_rho = mem.template dalloc<T>(m, st);
            if (!rs_rho1) rs_rho1 = mem.template dalloc<T>(m, st);
            rho_scale.assign(sc, sc + m);
            ldl->set_row_rho(rs_rho, rs_rho1);
        }
        factor_valid = false; rs_base = 0;   // the factor belongs to the previous scale
    }
    void factorize(double rho, double sigma) {   // numeric only, on the frozen pattern
        factor_valid = false;
        ++num_factorizations;
        ldl->factorize(rho, sigma);
        factor_valid = true; fac_rho = rho; fac_sigma = sigma;
    }

  protected:
    void check_params(const qps_params& p) override {
        if (p.adptRho) throw QpsError(QPS_ERR_UNSUPPORTED, "sparse shared-matrix batch: adptRho is not supported (one factor serves every column, so the per-problem rule cannot "
                                                           "run; qps_set_shared_adaptive_rho turns on the family-wide rule)");
        if (p.polish) throw QpsError(QPS_ERR_UNSUPPORTED, "sparse shared-matrix batch: polish is not supported");
        if (p.linsys != QPS_LINSYS_AUTO && p.linsys != QPS_LINSYS_KKT_LDL) throw QpsError(QPS_ERR_UNSUPPORTED, "sparse shared-matrix batch: linsys must be QPS_LINSYS_AUTO or QPS_LINSYS_KKT_LDL");
    }
    void factor_at_setup(double rho, double sigma, const qps_params&) override { factorize(rho, sigma); }
    void begin_solve(int warm, double, double, double) override {
        HIPC(hipMemsetAsync(xp, 0, sizeof(T) * (size_t)CP * (size_t)n, st));                        // :38
        if (warm == 0) { for (T* v : {z, zp, y}) HIPC(hipMemsetAsync(v, 0, sizeof(T) * (size_t)CP * (size_t)m, st)); }   // :39-41
        else HIPC(hipMemsetAsync(zp, 0, sizeof(T) * (size_t)CP * (size_t)m, st));                   // z (mode 1) and y stay; the first right-hand side is built from them (rhs_ready)
        if (warm == 2) { ProfScope ps(prof, cat_start, 1); csr_panel<T>(st, A, x, (int)n, z, (int)m, npanel); }   // OSQP's warm_start(x, y): z = A x~ without projection
        this->push_active();
        s = LdlPanelState<T>(); s.x = x; s.xp = xp; s.q = q; s.z = z; s.zp = zp; s.y = y; s.l = l; s.u = u; s.active = d_active; s.npanel = npanel;
        rhs_ready = false;
    }
    void switch_rho(double rho, double sigma) override {
        if (!rho_scale.empty()) this->push_row_rho(rho);                                            // the numeric factorisation reads rho_i
        factorize(rho, sigma);                                                                      // changedΡ
        rhs_ready = false;                                                                          // the right-hand side left behind holds 1 / rho of the previous rho
    }
    void iterate(int lvl, double rho, double sigma, double alpha) override {
        pf.lvl = lvl;
        ldl->iterate_panels(s, alpha, rho, sigma, rhs_ready, pf);                                   // LinearSystemSolvers.jl:37-40, SolveQuadraticProgram.jl:56-61
        rhs_ready = true;
    }
    void check_products(const T* xv, const T* yv) override {
        csr_panel<T>(st, A, xv, (int)n, Ax, (int)m, npanel);
        csr_panel<T>(st, P, xv, (int)n, Px, (int)n, npanel);
        csr_panel<T>(st, At, yv, (int)m, Aty, (int)n, npanel);
    }
};

// =================================================================================================================
// Matrix-free CG path (a scenario sweep on a model whose pattern fills in under any ordering).  No factor: every ADMM iteration runs LinOpCg!
// (LinearSystemSolvers.jl:164-186) for all columns in lockstep on 16-column panels (k_cg_panel.hip) -- the indices and values of P, A and A' are read once per
// CG iteration for 16 QPs and the launch chain of an iteration is paid once per batch.  Every column keeps its own cg! scalars on the device; the host reads
// them once per burst of iterations and a column that is done turns into a no-op.  A rho switch costs nothing, the per-row rho scale is a multiplier in the
// epilogue of A u.  Panels are n and m rows long, without padding rows.
// =================================================================================================================
template <typename T> struct CgSharedBatchSolver final : SharedFamilySolver<T> {
    using B = SharedFamilySolver<T>;
    using B::device; using B::n; using B::m; using B::count; using B::prof; using B::mem; using B::st; using B::CP; using B::npanel;
    using B::q; using B::l; using B::u; using B::x; using B::xp; using B::z; using B::zp; using B::y; using B::Ax; using B::Px; using B::Aty;
    using B::d_active; using B::active; using B::factor_valid; using B::fac_rho; using B::fac_sigma;
    using B::cat_chk; using B::cat_fac; using B::cat_switch; using B::cat_start; using B::rho_scale; using B::rs_rho; using B::rs_rho1; using B::rs_base;
    CgPanelArgs<T> a;                      // the matrices, the panels and the scalars of the launches
    T* w = nullptr;
    CgPanelState* h_state = nullptr;       // pinned: [0, CP) the scalars after the last burst, [CP, 2 CP) those cg! started from
    std::vector<int64_t> cg_total;         // per column, over the ADMM iterations of the running solve
    int last_cg = 0; double eps_pcg = 1e-6; int itr_pcg = 1000;
    int cat_rhs = 0, cat_it = 0, cat_post = 0;
    // qps_update_shared_matrices_csc: the canonical pattern the handle was created on (the values are not kept), and from the first update on the staging of the
    // new values and the position of every entry of the by-rows copy of A in CSC order
    std::vector<int64_t> hPcp, hPri, hAcp, hAri; double* upd_src = nullptr; int* upd_map = nullptr;

    CgSharedBatchSolver(int dev, int cnt, int64_t n_, int64_t m_, CgSharedInput&& in, const double* qh, const double* lh, const double* uh)
        : B(dev, cnt, n_, m_, (int)n_, (int)m_) {
        layout::CsrHost Ph, Ah, Ath;
        try {
            Ph = layout::csc_as_transposed_csr(n, n, in.Pcp, in.Pri, in.Pnz);      // P: CSC == CSR (symmetric, full storage)
            layout::csc_to_csr_pair(m, n, in.Acp, in.Ari, in.Anz, Ah, Ath);        // rows of A by a counting sort; rows of A' are the columns of A
        } catch (const std::length_error& ex) { throw QpsError(QPS_ERR_BAD_DIMENSION, ex.what()); }
        const int64_t pnnz = (int64_t)in.Pnz.size(), annz = (int64_t)in.Anz.size();
        a.n = (int)n; a.m = (int)m; a.npanel = npanel;
        a.P = this->upload_csr(Ph); a.A = this->upload_csr(Ah); a.At = this->upload_csr(Ath);
        a.spr_op = cg_panel_op_spr(pnnz, annz, (int)n);
        hPcp = std::move(in.Pcp); hPri = std::move(in.Pri); hAcp = std::move(in.Acp); hAri = std::move(in.Ari);
        const int64_t pn = (int64_t)CP * n, pm = (int64_t)CP * m;
        q = mem.template dalloc<T>(pn, st); x = mem.template dalloc<T>(pn, st); xp = mem.template dalloc<T>(pn, st); Px = mem.template dalloc<T>(pn, st);
        Aty = mem.template dalloc<T>(pn, st);
        l = mem.template dalloc<T>(pm, st); u = mem.template dalloc<T>(pm, st); z = mem.template dalloc<T>(pm, st); zp = mem.template dalloc<T>(pm, st);
        y = mem.template dalloc<T>(pm, st); Ax = mem.template dalloc<T>(pm, st);   // (dalloc zero-fills: z and y are defined from creation on, as qps_set_shared_warm_start needs)
        a.xx = mem.template dalloc<T>(pn, st); a.r = mem.template dalloc<T>(pn, st); a.u = mem.template dalloc<T>(pn, st); a.c = mem.template dalloc<T>(pn, st);
        a.t = mem.template dalloc<T>(pn, st); a.v = mem.template dalloc<T>(pm, st); a.w = w = mem.template dalloc<T>(pm, st);
        a.part_uc = mem.template dalloc<double>((int64_t)CP * cg_panel_op_blocks((int)n, a.spr_op), st);
        a.part_rr = mem.template dalloc<double>((int64_t)CP * cg_panel_vec_blocks((int)n), st);
        a.state = mem.template dalloc<CgPanelState>(2 * (int64_t)CP, st);
        h_state = mem.template pinned<CgPanelState>(2 * (size_t)CP);
        this->alloc_check_buffers();
        a.q = q; a.lo = l; a.hi = u; a.x = x; a.xp = xp; a.z = z; a.zp = zp; a.y = y; a.active = d_active;
        // algorithmic bytes per launch group, counted as the sparse path counts them: every matrix entry's index and value once per panel, the line it gathers
        // and the vectors read and written once per column
        const double sz = sizeof(T), c = CP, np = npanel, ents = (double)(pnnz + 2 * annz);
        cat_rhs = prof.category("cg shared: rhs, r0 = t - Op(x~) (panels)", np * ents * (sz + 4) + sz * c * (ents + 8.0 * n + 4.0 * m));
        cat_it = prof.category("cg shared: CG iteration (4 launches)", np * ents * (sz + 4) + sz * c * (ents + 11.0 * n + m));
        cat_post = prof.category("cg shared: post + update (panels)", np * annz * (sz + 4) + sz * c * (annz + 4.0 * n + 7.0 * m));
        cat_chk = prof.category("cg shared: check (A x, P x, A'y, norms)", np * ents * (sz + 4) + sz * c * (ents + 8.0 * n + 6.0 * m));
        this->cat_inf = prof.category("cg shared: infeasibility (deltas, 3 products, sums)", np * ents * (sz + 4) + sz * c * (ents + 10.0 * n + 10.0 * m));
        cat_fac = prof.category("cg shared: setup (nothing to factor)", 0.0);
        cat_switch = prof.category("cg shared: rho switch (rho_i only)", sz * 2.0 * m);
        cat_start = prof.category("cg shared: warm start (A x -> z)", np * annz * (sz + 4) + sz * c * (annz + m));
        this->update_vectors(qh, lh, uh);
    }
    ~CgSharedBatchSolver() override { this->drain(); }
    bool takes_csc() const override { return true; }
    void update_matrices(const double*, int64_t, const double*, int64_t) override {
        throw QpsError(QPS_ERR_UNSUPPORTED, "qps_update_shared_matrices: a CG shared-matrix batch takes its matrices through qps_update_shared_matrices_csc");
    }
    // New values on the frozen pattern of the three CSR copies the operator and the check read; nothing is factorised on this path
    void update_matrices_csc(const CanonicalCsc& Pc, const CanonicalCsc& Ac) override {
        if (!Pc.given && !Ac.given) return;
        HIPC(hipSetDevice(device));
        HIPC(hipStreamSynchronize(st));
        require_same_pattern("P", n, hPcp, hPri, Pc);
        require_same_pattern("A", n, hAcp, hAri, Ac);
        const int64_t pnnz = (int64_t)hPri.size(), annz = (int64_t)hAri.size();
        if (!upd_src) upd_src = mem.template dalloc<double>(pnnz + annz, st);
        if (!upd_map) {
            const std::vector<int> map = layout::csc_rows_position_map(m, n, hAcp, hAri);
            upd_map = mem.template dalloc<int>(annz, st);
            if (annz > 0) this->up->copy(upd_map, map.data(), sizeof(int) * (size_t)annz);
        }
        if (Pc.given && pnnz > 0) {
            this->up->copy(upd_src, Pc.nz.data(), sizeof(double) * (size_t)pnnz);
            refresh_values<T>(st, upd_src, nullptr, nullptr, pnnz, const_cast<T*>(a.P.va));
        }
        if (Ac.given && annz > 0) {
            this->up->copy(upd_src + pnnz, Ac.nz.data(), sizeof(double) * (size_t)annz);
            refresh_values<T>(st, upd_src + pnnz, upd_map, nullptr, annz, const_cast<T*>(a.A.va));
            refresh_values<T>(st, upd_src + pnnz, nullptr, nullptr, annz, const_cast<T*>(a.At.va));
        }
        HIPC(hipStreamSynchronize(st));
        factor_valid = false;
        this->last_conv.clear();
    }
    void set_equilibration(int passes) override {
        if (passes > 0) throw QpsError(QPS_ERR_UNSUPPORTED, "CG shared-matrix batch: equilibration is not supported");
    }
    void set_rho_scale(const double* sc) override {
        HIPC(hipSetDevice(device));
        HIPC(hipStreamSynchronize(st));
        if (!sc) {
            for (T** v : {&rs_rho, &rs_rho1}) { mem.release(*v); *v = nullptr; }
            rho_scale.clear();
        } else {
            if (!rs_rho) rs_rho = mem.template dalloc<T>(m, st);
            if (!rs_rho1) rs_rho1 = mem.template dalloc<T>(m, st);
            rho_scale.assign(sc, sc + m);
        }
        rs_base = 0;
    }

  protected:
    void check_params(const qps_params& p) override {
        if (p.adptRho) throw QpsError(QPS_ERR_UNSUPPORTED, "CG shared-matrix batch: adptRho is not supported (the columns run in lockstep on one rho, so the per-problem rule "
                                                           "cannot run; qps_set_shared_adaptive_rho turns on the family-wide rule)");
        if (p.polish) throw QpsError(QPS_ERR_UNSUPPORTED, "CG shared-matrix batch: polish is not supported");
        if (p.linsys != QPS_LINSYS_AUTO && p.linsys != QPS_LINSYS_CG) throw QpsError(QPS_ERR_UNSUPPORTED, "CG shared-matrix batch: linsys must be QPS_LINSYS_AUTO or QPS_LINSYS_CG");
        if (!(p.epsPcg >= 0) || !std::isfinite(p.epsPcg)) throw QpsError(QPS_ERR_BAD_ARGUMENT, "CG shared-matrix batch: epsPcg must be finite and >= 0");
        if (p.numItrPcg < 1) throw QpsError(QPS_ERR_BAD_ARGUMENT, "CG shared-matrix batch: numItrPcg must be >= 1");
        eps_pcg = p.epsPcg; itr_pcg = p.numItrPcg;
    }
    void factor_at_setup(double rho, double sigma, const qps_params&) override { factor_valid = true; fac_rho = rho; fac_sigma = sigma; }   // LinOpCgInit: nothing to factor
    void begin_solve(int warm, double, double, double) override {
        for (T* v : {xp, a.xx}) HIPC(hipMemsetAsync(v, 0, sizeof(T) * (size_t)CP * (size_t)n, st));   // :38; LinearSystemSolvers.jl:147: x~ starts from zero at every solve
        if (warm == 0) { for (T* v : {z, zp, y}) HIPC(hipMemsetAsync(v, 0, sizeof(T) * (size_t)CP * (size_t)m, st)); }   // :39-41
        else HIPC(hipMemsetAsync(zp, 0, sizeof(T) * (size_t)CP * (size_t)m, st));                   // z (mode 1) and y stay
        if (warm == 2) { ProfScope ps(prof, cat_start, 1); csr_panel<T>(st, a.A, x, (int)n, z, (int)m, npanel); }   // OSQP's warm_start(x, y): z = A x~ without projection
        this->push_active();
        cg_total.assign(count, 0);
        last_cg = 0;
        a.eps_pcg = eps_pcg; a.max_it = itr_pcg;
    }
    void switch_rho(double rho, double) override {
        if (!rho_scale.empty()) this->push_row_rho(rho);                                            // the operator and the row update read rho_i
    }
    void iterate(int lvl, double rho, double sigma, double alpha) override {
        const bool scaled = !rho_scale.empty();
        a.rho = (T)rho; a.sigma = (T)sigma; a.alpha = (T)alpha; a.rho_row = scaled ? rs_rho : nullptr; a.rho1_row = scaled ? rs_rho1 : nullptr;
        {
            ProfScope ps(prof, cat_rhs, lvl);
            panel_w<T>(st, z, y, d_active, a.rho_row, a.rho, (int)m, npanel, w);                    // LinearSystemSolvers.jl:176
            cg_panel_begin<T>(st, a);                                                               // :177-178 and the head of cg!
        }
        HIPC(hipMemcpyAsync(h_state + CP, a.state, sizeof(CgPanelState) * (size_t)CP, hipMemcpyDeviceToHost, st));   // read at the first synchronisation
        // Bursts as CgPlugin::cg sizes them: the first is the previous ADMM iteration's count, every further one what the slowest column's measured contraction
        // says is left; two at least (a synchronisation costs about one iteration), 64 at most, never past numItrPcg.  A column's arithmetic does not depend
        // on the burst: an iteration enqueued past its end is a no-op for it.
        int cur = 0, launched = 0, batch = std::min(std::max(2, std::min(last_cg, 64)), itr_pcg);
        for (;;) {
            for (int b = 0; b < batch; ++b) {
                ProfScope ps(prof, cat_it, lvl);
                cg_panel_iteration<T>(st, a, cur, b == 0);
                cur ^= 1;
            }
            cg_panel_finish<T>(st, a, cur);
            launched += batch;
            HIPC(hipMemcpyAsync(h_state, a.state + (int64_t)cur * CP, sizeof(CgPanelState) * (size_t)CP, hipMemcpyDeviceToHost, st));
            HIPC(hipStreamSynchronize(st));
            prof.harvest();
            int left = 0; bool running = false;
            for (int b = 0; b < count; ++b) {
                const CgPanelState &s0 = h_state[CP + b], &s1 = h_state[b];
                if (!active[b] || s1.done) continue;
                running = true;
                const double r0 = std::sqrt(s0.res2), r1 = std::sqrt(s1.res2);
                int lb = std::max(launched, 1);                                                     // no usable rate: as many again
                if (r1 > 0 && r0 > r1 && s1.tol > 0 && r1 > s1.tol) lb = (int)std::fmin(64.0, std::ceil(std::log(r1 / s1.tol) / (std::log(r0 / r1) / std::max(1, s1.itn))));
                left = std::max(left, lb);
            }
            if (!running || launched >= itr_pcg) break;
            batch = std::max(1, std::min(std::min(std::max(left, 2), std::max(launched, 2)), std::min(64, itr_pcg - launched)));
        }
        last_cg = 0;
        for (int b = 0; b < count; ++b) if (active[b]) { cg_total[b] += h_state[b].itn; last_cg = std::max(last_cg, h_state[b].itn); }
        { ProfScope ps(prof, cat_post, lvl); cg_panel_post<T>(st, a); }                             // :181; SolveQuadraticProgram.jl:56-61
    }
    void check_products(const T* xv, const T* yv) override {
        csr_panel<T>(st, a.A, xv, (int)n, Ax, (int)m, npanel);
        csr_panel<T>(st, a.P, xv, (int)n, Px, (int)n, npanel);
        csr_panel<T>(st, a.At, yv, (int)m, Aty, (int)n, npanel);
    }
    int64_t column_cg_iterations(int b) override { return b < (int)cg_total.size() ? cg_total[b] : 0; }
};

}  // namespace

int shared_batch_max_np(int dtype) { return 16 * 512 * (dtype == QPS_F64 ? VecOf<double>::N : VecOf<float>::N); }   // whole-factor explicit inverse: 16384 fp64 / 32768 fp32 (k_trsv.hip)

BatchSolverBase* make_dense_shared_batch(int device, int dtype, int count, int64_t n, int64_t m, const double* P, int64_t ldp, const double* A, int64_t lda,
                                         const double* q, const double* l, const double* u) {
    auto load = [&](auto s) { s->load(P, ldp, A, lda, q, l, u); return static_cast<BatchSolverBase*>(s.release()); };   // a unique_ptr: a throw while loading drops the solver
    if (dtype == QPS_F64) return load(std::make_unique<SharedBatchSolver<double>>(device, count, n, m));
    return load(std::make_unique<SharedBatchSolver<float>>(device, count, n, m));
}
BatchSolverBase* make_sparse_shared_batch(int device, int dtype, int count, int64_t n, int64_t m, SparseSharedInput&& in, const double* q, const double* l,
                                          const double* u) {
    if (dtype == QPS_F64) return new SparseSharedBatchSolver<double>(device, count, n, m, std::move(in), q, l, u);
    return new SparseSharedBatchSolver<float>(device, count, n, m, std::move(in), q, l, u);
}
BatchSolverBase* make_cg_shared_batch(int device, int dtype, int count, int64_t n, int64_t m, CgSharedInput&& in, const double* q, const double* l, const double* u) {
    if (dtype == QPS_F64) return new CgSharedBatchSolver<double>(device, count, n, m, std::move(in), q, l, u);
    return new CgSharedBatchSolver<float>(device, count, n, m, std::move(in), q, l, u);
}

}  // namespace qps
