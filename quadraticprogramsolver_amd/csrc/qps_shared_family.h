// qps_shared_family.h -- the shared-matrix batches: `count` QPs on ONE P and ONE A that differ in q, l, u only.  The one host driver of their ADMM loop
// (SharedFamilySolver: SolveQuadraticProgram.jl:36-73 for every column at once, every option of qps_set_shared_*, the polishing step) and the host checks its
// paths share.  Three linear-system paths derive from it: the dense Cholesky on MFMA panels (qps_shared_dense.hip), the sparse KKT L D L' and the matrix-free CG
// on the three CSR copies of CsrFamilySolver (qps_shared_csr.hip).  Host code only; a header template, compiled in both units.
#pragma once
#include <limits>
#include <memory>

#include "qps_batch.h"
#include "qps_polish.h"
#include "shared_family_rules.h"
#include "spmv_layout.h"

namespace qps {

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
// What the three paths have in common: the resources, the state in 16-column panels [panel][rows][16] (rows = rowsN for n-vectors, rowsM for m-vectors), the
// options, and the loop.  rho is common (a common factor needs a common rho): fixed, or moved for the whole family by qps_set_shared_adaptive_rho; on a path
// without a factor (takes_column_rho) qps_set_shared_column_rho lets every column move its own rho by SolveQuadraticProgram.jl:47, :92-96.  Every column
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

    // The eleven state panels of every path, then the check's buffers.  z and y are cleared here: the state qps_set_shared_warm_start continues from is defined
    // from creation on.
    void alloc_state_panels() {
        const int64_t pn = (int64_t)CP * rowsN, pm = (int64_t)CP * rowsM;
        for (T** v : {&q, &x, &xp, &Px, &Aty}) *v = mem.dalloc<T>(pn, st);
        for (T** v : {&l, &u, &z, &zp, &y, &Ax}) *v = mem.dalloc<T>(pm, st);
        for (T* v : {z, y}) HIPC(hipMemsetAsync(v, 0, sizeof(T) * (size_t)pm, st));
        alloc_check_buffers();
    }
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
    // the vectors the handle keeps between calls, in place: *= 2^(+-k) by the exponents in kd / ke (what both paths' apply_equilibration end with)
    void rescale_kept_vectors(int sign) {
        panel_rowscale<T>(st, q, kd, sign, rowsN, npanel, q);
        for (T* v : {l, u, z}) panel_rowscale<T>(st, v, ke, sign, rowsM, npanel, v);
        panel_rowscale<T>(st, y, ke, -sign, rowsM, npanel, y);
    }
    // rs_rho / rs_rho1 exist while a scale is set; the path's own part (what it derives from the scale, what goes stale) is rho_scale_changed
    void set_rho_scale(const double* s) override {
        HIPC(hipSetDevice(device));
        HIPC(hipStreamSynchronize(st));
        if (!s) {
            for (T** v : {&rs_rho, &rs_rho1}) { mem.release(*v); *v = nullptr; }
            rho_scale.clear();
        } else {
            if (!rs_rho) rs_rho = mem.dalloc<T>(rowsM, st);
            if (!rs_rho1) rs_rho1 = mem.dalloc<T>(rowsM, st);
            rho_scale.assign(s, s + m);
        }
        rs_base = 0;
        rho_scale_changed(s);
    }
    // the start state of a solve in warm start mode `warm`: SolveQuadraticProgram.jl:38, then :39-41 or, from mode 1 on, zp alone -- z (mode 1) and y stay, and
    // iteration 1 overwrites zp before a check reads it.  A path's begin_solve calls this and clears its own panels.
    void reset_state(int warm) {
        HIPC(hipMemsetAsync(xp, 0, sizeof(T) * (size_t)CP * rowsN, st));
        if (warm == 0) { for (T* v : {z, zp, y}) HIPC(hipMemsetAsync(v, 0, sizeof(T) * (size_t)CP * rowsM, st)); }
        else HIPC(hipMemsetAsync(zp, 0, sizeof(T) * (size_t)CP * rowsM, st));
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
        if ((family_rho || column_rho) && !(p.fctrRho > 0)) throw QpsError(QPS_ERR_BAD_ARGUMENT, "fctrRho must be positive");
        double rho = p.rho, rhorho = rho;                                                           // :43; rho moves under the family rule only
        const double sigma = p.sigma, alpha = p.alpha;
        const double epsAdmm = std::fmin(p.epsAbs, p.epsRel) * 1e-2;                                // SolveQuadraticProgram.jl:34
        const bool reuse = p.reuseFactor && factor_valid && fac_rho == rho && fac_sigma == sigma;
        if (!rho_scale.empty()) push_row_rho(column_rho ? 1.0 : rho);                               // under the column rule the rows hold s_i, rho_b is the column's
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
        const std::vector<int> alone(1, 1);                                                         // the mask of a family of one: the column rule's proposal
        if (column_rho) column_rho_changed(rho_col);                                                // :43 for every column
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
            if (column_rho) {                                                                       // :47, column by column; a column that stopped keeps its rho
                bool moved = false;
                for (int b = 0; b < count; ++b)
                    if (active[b] && ((prop_col[b] * p.fctrRho < rho_col[b]) || (prop_col[b] > p.fctrRho * rho_col[b]))) { rho_col[b] = prop_col[b]; ++nref[b]; moved = true; }
                if (moved) {
                    const double ta = now_s();
                    { ProfScope ps(prof, cat_switch, 1); column_rho_changed(rho_col); }
                    HIPC(hipStreamSynchronize(st));
                    tref += now_s() - ta;
                }
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
            if (column_rho)                                                                         // :92-96 from the column's own four norms, its stopping check included
                for (int b = 0; b < count; ++b) if (active[b] || iters[b] == ii) prop_col[b] = family_rho_proposal(res_host + 8 * b, alone, 1, rho_col[b], prop_col[b]);
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
    // qps_adjoint_shared: per column, K r = [g_x; 0] on the active rows of y -- the system of the polishing step under another right-hand side, by the same
    // refinement rounds -- then dq = -r_x, dl / du = r_lambda on the lower / upper active rows and, on a path that keeps a CSC pattern, the gradients with
    // respect to the stored values of P and A summed over the columns (value_gradients).  With the equilibration on the rounds run on the scaled data: the
    // right-hand side is D g_x, and r_x = D r~_x, r_lambda = E r~_lambda are exact; in the unscaled r, x, y every formula holds in the caller's units.  A column
    // whose last MINRES call did not converge gives zeros and is left out of the sums.  Work panels of this call only; nothing the handle keeps is written.
    void adjoint(const double* xh, const double* yh, const double* gxh, const qps_params& p, double* dq, double* dl, double* du, double* dPv, double* dAv,
                 qps_polish_report* reports) override {
        const bool mats = dPv || dAv;
        if (mats && !this->takes_csc())
            throw QpsError(QPS_ERR_UNSUPPORTED, "qps_adjoint_shared: a dense shared-matrix batch gives no gradients with respect to the matrices (dP_nzval and "
                                                "dA_nzval must be NULL)");
        HIPC(hipSetDevice(device));
        const double t0 = now_s();
        const int64_t pn = (int64_t)CP * rowsN, pm = (int64_t)CP * rowsM;
        DeviceOwner wm;
        T* gb = wm.dalloc<T>(pn, st); T* xb = mats ? wm.dalloc<T>(pn, st) : nullptr; T* yb = (yh || (mats && kd)) ? wm.dalloc<T>(pm, st) : nullptr;
        T* out = wm.dalloc<T>(pn + 2 * pm, st);
        put_panels(gxh, gb, n, rowsN);
        if (kd) panel_rowscale<T>(st, gb, kd, 1, rowsN, npanel, gb);                                // D g_x
        if (mats) put_panels(xh, xb, n, rowsN);                                                     // x and y stay in the caller's units: only the sign of y
        if (yh) put_panels(yh, yb, m, rowsM);                                                       // enters the system, and E keeps it
        else if (yb) panel_rowscale<T>(st, y, ke, 1, rowsM, npanel, yb);                            // y = E y~
        const T* ypan = yb ? yb : y;
        std::vector<PolishReport> reps(count, PolishReport());
        PolishWork w;
        polish_work_alloc(w, std::vector<int>());
        shared_adjoint_setup<T>(st, w.g, gb, ypan, w.mask, w.gv, w.counts);
        polish_fetch_counts(w);
        polish_rounds(w, p, reps);
        T* tl = w.t + pn;
        if (kd) { panel_rowscale<T>(st, w.t, kd, 1, rowsN, npanel, w.t); panel_rowscale<T>(st, tl, ke, 1, rowsM, npanel, tl); }   // r_x = D r~_x, r_lambda = E r~_lambda
        shared_adjoint_readout<T>(st, w.g, w.live_dev, ypan, w.t, out, out + pn, out + pn + pm);
        if (dq) get_panels(out, dq, n, rowsN);
        if (dl) get_panels(out + pn, dl, m, rowsM);
        if (du) get_panels(out + pn + pm, du, m, rowsM);
        if (mats) value_gradients(w.t, xb, tl, ypan, dPv, dAv);
        HIPC(hipStreamSynchronize(st));
        const double secs = now_s() - t0;
        for (int b = 0; b < count && reports; ++b) {
            qps_polish_report& r = reports[b];
            r.flag = reps[b].flag; r.refinements = reps[b].refinements; r.minresIterations = reps[b].minresIterations; r.numActiveLower = w.hi[2 * b];
            r.numActiveUpper = w.hi[2 * b + 1]; r.reserved0 = 0; r.relres = reps[b].relres; r.seconds = secs;
        }
    }
    // The work panels of one run of the refinement rounds (polish_panels, adjoint): the KKT vectors gv (the right-hand side g), t (the solution) and the seven
    // of MINRES, the mask and wl, the partial sums, the per-column states and counts and their pinned copies.  They live for one call.
    struct PolishWork {
        DeviceOwner wm;
        SharedPolishGeom g;
        T *gv = nullptr, *t = nullptr, *tt = nullptr, *rhs = nullptr, *c = nullptr, *r1 = nullptr, *r2 = nullptr, *w1 = nullptr, *w2 = nullptr, *mask = nullptr, *wl = nullptr;
        double *pa = nullptr, *pb = nullptr; SharedPolishState *state = nullptr, *hs = nullptr; int *counts = nullptr, *live_dev = nullptr, *hi = nullptr;
        std::vector<int> live; int nlive = 0;
    };
    void polish_work_alloc(PolishWork& w, const std::vector<int>& take) {
        SharedPolishGeom& g = w.g; g.n = (int)n; g.m = (int)m; g.rowsN = rowsN; g.rowsM = rowsM; g.npanel = npanel;
        const int64_t N = (int64_t)CP * (rowsN + rowsM), ML = (int64_t)CP * rowsM; const int nblk = shared_polish_blocks(rowsN, rowsM);
        w.gv = w.wm.template dalloc<T>(9 * N + 2 * ML, st);
        w.t = w.gv + N; w.tt = w.t + N; w.rhs = w.tt + N; w.c = w.rhs + N; w.r1 = w.c + N; w.r2 = w.r1 + N; w.w1 = w.r2 + N; w.w2 = w.w1 + N;   // t = tt = 0 (:307-308)
        w.mask = w.w2 + N; w.wl = w.mask + ML;
        w.pa = w.wm.template dalloc<double>(2 * (int64_t)CP * nblk, st); w.pb = w.pa + (int64_t)CP * nblk;
        w.state = w.wm.template dalloc<SharedPolishState>(2 * (int64_t)CP, st);
        w.counts = w.wm.template dalloc<int>(3 * (int64_t)CP, st); w.live_dev = w.counts + 2 * CP;
        w.hs = w.wm.template pinned<SharedPolishState>((size_t)CP); w.hi = w.wm.template pinned<int>(3 * (size_t)CP);
        w.live.assign(CP, 0);
        w.nlive = 0;
        for (int b = 0; b < count; ++b) w.nlive += w.live[b] = take.empty() || take[b];
    }
    void polish_push_live(PolishWork& w) {
        for (int b = 0; b < CP; ++b) w.hi[2 * CP + b] = w.live[b];
        HIPC(hipMemcpyAsync(w.live_dev, w.hi + 2 * CP, sizeof(int) * CP, hipMemcpyHostToDevice, st));
        HIPC(hipStreamSynchronize(st));
    }
    // what follows the set-up kernel of either caller: the active-set counts on their way to the host, then the first mask of live columns
    void polish_fetch_counts(PolishWork& w) {
        HIPC(hipMemcpyAsync(w.hi, w.counts, sizeof(int) * 2 * CP, hipMemcpyDeviceToHost, st));
        polish_push_live(w);
    }
    // SolveQuadraticProgram.m:289-325 for the columns of `take` (empty: all), all at once, on the data the handle holds (the scaled data while the equilibration
    // is on): ypan are rowsM panels, xpan rowsN panels that take t_x where the column's last MINRES call converged.  Three parts: the set-up of mask and
    // right-hand side, the refinement rounds (polish_rounds) and the read-out.  The work panels live for this call only.
    void polish_panels(const T* ypan, T* xpan, const qps_params& p, const std::vector<int>& take, std::vector<PolishReport>& reps) {
        const double t0 = now_s();
        reps.assign(count, PolishReport());
        if (p.numItrPolish <= 0) return;                                                            // :292
        PolishWork w;
        polish_work_alloc(w, take);
        shared_polish_setup<T>(st, w.g, q, l, u, ypan, w.mask, w.gv, w.counts);                     // :293-299
        polish_fetch_counts(w);
        polish_rounds(w, p, reps);
        shared_polish_select<T>(st, w.g, w.live_dev, w.t, xpan);                                    // :322-325
        HIPC(hipStreamSynchronize(st));
        const double secs = now_s() - t0;
        for (int b = 0; b < count; ++b) { reps[b].numLower = w.hi[2 * b]; reps[b].numUpper = w.hi[2 * b + 1]; reps[b].seconds = secs; }
    }
    // The refinement rounds :314-320 of K t = g from t = 0, for the mask and the right-hand side gv a set-up kernel left in `w`.  K v comes from check_products --
    // the matrices are read once per MINRES iteration for all columns of a panel pair -- and k_shared_polish.hip does the rest.  The columns advance in lockstep:
    // in round jj those still refining form g - K t and run MINRES together, the host reading the per-column states every 8 iterations; a column whose call
    // ended with flag 1 leaves (:316-318), the others add tt and go on.  On return w.t holds t, and w.live / w.live_dev name the columns whose last call converged.
    void polish_rounds(PolishWork& w, const qps_params& p, std::vector<PolishReport>& reps) {
        const SharedPolishGeom& g = w.g;
        T *const gv = w.gv, *const t = w.t, *const tt = w.tt, *const rhs = w.rhs, *const c = w.c, *const mask = w.mask, *const wl = w.wl;
        T *r1 = w.r1, *r2 = w.r2, *w1 = w.w1, *w2 = w.w2;
        double *const pa = w.pa, *const pb = w.pb; SharedPolishState *const state = w.state, *const hs = w.hs; int* const live_dev = w.live_dev;
        std::vector<int>& live = w.live; int& nlive = w.nlive;
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
            polish_push_live(w);
            if (nlive > 0) shared_polish_add<T>(st, g, live_dev, state + (int64_t)cur * CP, t, tt); // :319
        }
        for (int b = 0; b < count; ++b) live[b] = reps[b].flag == 0;
        polish_push_live(w);
    }

  protected:
    virtual void check_params(const qps_params& p) = 0;                               // the path's refusals
    virtual void factor_at_setup(double rho, double sigma, const qps_params& p) = 0;  // no reusable factor: LinSysSolInit for (rho, sigma)
    // Zero the start state for warm start mode `warm` (the path's panels included), call push_active(), run the mode 1 / 2 start launches under cat_start and
    // prepare the launch arguments of this solve.
    virtual void begin_solve(int warm, double rho, double sigma, double alpha) = 0;
    virtual void switch_rho(double rho, double sigma) = 0;                            // the family moved to `rho`: new factor, state that held the previous rho
    // qps_set_shared_column_rho: column b runs on rho_col[b] from the next iteration on (at the start of a solve: every column on params.rho).  Only a path
    // that answers takes_column_rho is ever asked; it leaves the host vector free when it returns.
    virtual void column_rho_changed(const std::vector<double>& /*rho_col*/) {}
    virtual void iterate(int lvl, double rho, double sigma, double alpha) = 0;        // one ADMM iteration of every active column, profiled at level `lvl`
    // Ax = A xv, Px = P xv, Aty = A'yv for arbitrary panels (the check's x, y; the certificates' dx, dyh; the polishing step's v_x, mask v_lambda); usable outside a solve
    virtual void check_products(const T* xv, const T* yv) = 0;
    // qps_adjoint_shared on a path that keeps a CSC pattern: dP [nnz(P)] and dA [nnz(A)] (either may be null) in the order of that pattern, from the unscaled
    // panels r_x, x (n rows) and r_lambda, y (m rows) whose padding columns and failed columns of r are zero.  Only such a path is ever asked.
    virtual void value_gradients(const T* /*rx*/, const T* /*xv*/, const T* /*rl*/, const T* /*yv*/, double* /*dP*/, double* /*dA*/) {}
    virtual int64_t column_cg_iterations(int) { return 0; }                           // qps_info.cgIterations of column b of the running solve (a path without CG: 0)
    // set_rho_scale replaced the scale by `s` ([m], or NULL: none), stream idle: what the path keeps beside rs_rho / rs_rho1, and what it invalidates
    virtual void rho_scale_changed(const double* /*s*/) {}
};

}  // namespace qps
