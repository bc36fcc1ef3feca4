// qps_shared_csr.hip -- the two paths of the shared-matrix batches that are created from CSC arrays, under the family driver of qps_shared_family.h:
// CsrFamilySolver (the three CSR copies the check reads, the frozen pattern, qps_update_shared_matrices_csc and the values-only qps_update_shared_values with its
// tests on the device), the sparse KKT L D L' with panel sweeps
// (SparseSharedBatchSolver, k_ldl.hip, k_csr_panel.hip) and the matrix-free CG on panels (CgSharedBatchSolver, k_cg_panel.hip).
// qps_capi.hip validates the caller's arrays and builds the handles through the two factories at the end of this file.
#include <cstring>

#include "qps_ldl.h"
#include "qps_shared_family.h"

namespace qps {
namespace {

// =================================================================================================================
// What the sparse and the CG path have in common: P, A and A' as CSR x panel matrices (k_csr_panel.hip: the check's products; the CG path's operator), the
// canonical CSC pattern the handle was created on, and the replacement of the values on that pattern.  Panels are n and m rows long, without padding rows.
// =================================================================================================================
template <typename T> struct CsrFamilySolver : SharedFamilySolver<T> {
    using B = SharedFamilySolver<T>;
    using B::device; using B::n; using B::m; using B::prof; using B::mem; using B::st; using B::up; using B::npanel;
    using B::x; using B::z; using B::Ax; using B::Px; using B::Aty; using B::factor_valid; using B::cat_start;
    CsrPanelMatrix<T> P, A, At;
    std::vector<int64_t> hPcp, hPri, hAcp, hAri;   // the pattern; the values stay with the path that needs them
    // qps_update_shared_matrices_csc, from its first call on: the staging of the canonical values (nnz(P) + nnz(A) doubles) and the position of every entry of
    // the by-rows copy of A in CSC order
    double* upd_src = nullptr; int* upd_map = nullptr;
    // qps_update_shared_values, from its first call on: where the transpose partner of every entry of P is stored (-1: nowhere), the verdict block of
    // validate_values for P and for A on the device and pinned, and the three profiling categories of the call
    int* upd_partner = nullptr; unsigned long long *upd_verdict = nullptr, *h_verdict = nullptr;
    int cat_upd_stage = 0, cat_upd_check = 0, cat_upd_refresh = 0;
    // qps_adjoint_shared, from its first call with a matrix gradient on: the row of every entry of the CSR copies P and A' (for both the column of the entry in
    // the canonical CSC pattern), and the profiling category of the value kernel
    int *adj_rowP = nullptr, *adj_rowAt = nullptr; int cat_adj_values = 0;
    const char* const path_word;   // "a sparse", "a CG": how the refusal of the dense form names the path

    CsrFamilySolver(int dev, int cnt, int64_t n_, int64_t m_, const char* word, std::vector<int64_t>&& Pcp, std::vector<int64_t>&& Pri, const std::vector<double>& Pnz,
                    std::vector<int64_t>&& Acp, std::vector<int64_t>&& Ari, const std::vector<double>& Anz)
        : B(dev, cnt, n_, m_, (int)n_, (int)m_), path_word(word) {
        layout::CsrHost Ph, Ah, Ath;
        try {
            Ph = layout::csc_as_transposed_csr(n, n, Pcp, Pri, Pnz);      // P: CSC == CSR (symmetric, full storage)
            layout::csc_to_csr_pair(m, n, Acp, Ari, Anz, Ah, Ath);        // rows of A by a counting sort; rows of A' are the columns of A
        } catch (const std::length_error& ex) { throw QpsError(QPS_ERR_BAD_DIMENSION, ex.what()); }
        P = this->upload_csr(Ph); A = this->upload_csr(Ah); At = this->upload_csr(Ath);
        hPcp = std::move(Pcp); hPri = std::move(Pri); hAcp = std::move(Acp); hAri = std::move(Ari);
    }
    int64_t nnzP() const { return (int64_t)hPri.size(); }   // stored entries of P and of A: the one place the paths read them from
    int64_t nnzA() const { return (int64_t)hAri.size(); }
    bool takes_csc() const override { return true; }
    void update_matrices(const double*, int64_t, const double*, int64_t) override {
        throw QpsError(QPS_ERR_UNSUPPORTED, std::string("qps_update_shared_matrices: ") + path_word +
                                                " shared-matrix batch takes its matrices through qps_update_shared_matrices_csc");
    }
    // New values on the frozen pattern: one upload of the canonical values as doubles, then one launch per value array (the CSR copies P, A, A'; on the sparse
    // path the factor's [P; A]) that rounds, permutes and scales.  upd_src and upd_map are built at the first update and kept.
    void update_matrices_csc(const CanonicalCsc& Pc, const CanonicalCsc& Ac) override {
        if (!Pc.given && !Ac.given) return;
        HIPC(hipSetDevice(device));
        HIPC(hipStreamSynchronize(st));
        require_same_pattern("P", n, hPcp, hPri, Pc);
        require_same_pattern("A", n, hAcp, hAri, Ac);
        check_new_values(Pc, Ac);
        const int64_t np = nnzP(), na = nnzA();
        if (!upd_src) upd_src = mem.template dalloc<double>(np + na, st);
        if (!upd_map) {
            const std::vector<int> map = layout::csc_rows_position_map(m, n, hAcp, hAri);
            upd_map = mem.template dalloc<int>(na, st);
            if (na > 0) up->copy(upd_map, map.data(), sizeof(int) * (size_t)na);
        }
        const int* eK = update_exponents();
        const int *eP = eK ? eK + np + na : nullptr, *eA = eK ? eP + np : nullptr, *eAt = eK ? eA + na : nullptr;
        if (Pc.given && np > 0) {
            up->copy(upd_src, Pc.nz.data(), sizeof(double) * (size_t)np);
            refresh_values<T>(st, upd_src, nullptr, eP, np, const_cast<T*>(P.va));
            values_replaced(false, upd_src, eK, np, Pc.nz.data());
        }
        if (Ac.given && na > 0) {
            up->copy(upd_src + np, Ac.nz.data(), sizeof(double) * (size_t)na);
            refresh_values<T>(st, upd_src + np, upd_map, eA, na, const_cast<T*>(A.va));
            refresh_values<T>(st, upd_src + np, nullptr, eAt, na, const_cast<T*>(At.va));
            values_replaced(true, upd_src + np, eK ? eK + np : nullptr, na, Ac.nz.data());
        }
        HIPC(hipStreamSynchronize(st));
        factor_valid = false;                                      // the next solve runs the path's setup on the new values, also with reuseFactor
        this->last_conv.clear();
    }
    void get_pattern(int64_t* np, int64_t* na, int64_t* Pcp, int64_t* Pri, int64_t* Acp, int64_t* Ari) override {
        if (np) *np = nnzP();
        if (na) *na = nnzA();
        if (Pcp) std::copy(hPcp.begin(), hPcp.end(), Pcp);
        if (Pri) std::copy(hPri.begin(), hPri.end(), Pri);
        if (Acp) std::copy(hAcp.begin(), hAcp.end(), Acp);
        if (Ari) std::copy(hAri.begin(), hAri.end(), Ari);
    }
    // New values in the order of the frozen pattern, nothing else from the caller: the host looks at the two counts and, for device input, at the pointer
    // attributes; the values go into the staging (an upload, or a device-to-device copy on the handle's stream) and validate_values tests them there -- finite,
    // issymmetric(mP) with tolerance 0, the range under kept exponents -- into one verdict block that the host reads with one copy and one synchronisation.
    // Only a clean verdict reaches the launches of update_matrices_csc.  upd_partner (the transpose partner of every entry of P) and the verdict block are
    // built at the first call and kept, like upd_src and upd_map; they and the staging are all a refused call leaves behind.
    ValuesVerdict update_values(const double* Pv, int64_t cntP, const double* Av, int64_t cntA, int location) override {
        const int64_t np = nnzP(), na = nnzA();
        auto count_is = [](const char* name, int64_t got, int64_t want) {
            if (got == want) return;
            char b[192];
            snprintf(b, sizeof b, "qps_update_shared_values: nnz%s is %lld, the handle's %s has %lld stored entries; the handle is unchanged", name, (long long)got,
                     name, (long long)want);
            throw QpsError(QPS_ERR_BAD_ARGUMENT, b);
        };
        if (Pv) count_is("P", cntP, np);
        if (Av) count_is("A", cntA, na);
        if (!Pv && !Av) return {};
        HIPC(hipSetDevice(device));
        // device input: what the pointers are is decided here, on the host, before anything is enqueued
        if (location == QPS_MEM_DEVICE) {
            if (Pv && np > 0) require_device_memory("P_nzval", Pv);
            if (Av && na > 0) require_device_memory("A_nzval", Av);
        }
        HIPC(hipStreamSynchronize(st));
        if (!upd_src) upd_src = mem.template dalloc<double>(np + na, st);
        if (!upd_map) {
            const std::vector<int> map = layout::csc_rows_position_map(m, n, hAcp, hAri);
            upd_map = mem.template dalloc<int>(na, st);
            if (na > 0) up->copy(upd_map, map.data(), sizeof(int) * (size_t)na);
        }
        if (!upd_partner) {
            const std::vector<int> map = layout::csc_transpose_partner_map(n, hPcp, hPri);
            upd_partner = mem.template dalloc<int>(np, st);
            if (np > 0) up->copy(upd_partner, map.data(), sizeof(int) * (size_t)np);
            upd_verdict = mem.template dalloc<unsigned long long>(2 * VALIDATE_VERDICT_KEYS, st);
            h_verdict = mem.template pinned<unsigned long long>(2 * VALIDATE_VERDICT_KEYS);
            cat_upd_stage = prof.category("shared values: staging (upload / device copy)", 8.0 * (np + na));
            cat_upd_check = prof.category("shared values: validation + verdict", 8.0 * (np + na));
            cat_upd_refresh = prof.category("shared values: refresh of the value arrays", (8.0 + sizeof(T)) * (np + 2.0 * na));
        }
        const int* eK = update_exponents();
        const int *eP = eK ? eK + np + na : nullptr, *eA = eK ? eP + np : nullptr, *eAt = eK ? eA + na : nullptr;
        const bool doP = Pv && np > 0, doA = Av && na > 0;
        {
            ProfScope ps(prof, cat_upd_stage, 1);
            if (doP) stage_values(upd_src, Pv, np, location);
            if (doA) stage_values(upd_src + np, Av, na, location);
        }
        {
            ProfScope ps(prof, cat_upd_check, 1);
            HIPC(hipMemsetAsync(upd_verdict, 0, sizeof(unsigned long long) * 2 * VALIDATE_VERDICT_KEYS, st));
            if (doP) validate_values<T>(st, upd_src, np, upd_partner, P.rp, P.ci, (int)n, eK, upd_verdict);
            if (doA) validate_values<T>(st, upd_src + np, na, nullptr, nullptr, nullptr, (int)n, eK ? eK + np : nullptr, upd_verdict + VALIDATE_VERDICT_KEYS);
            HIPC(hipMemcpyAsync(h_verdict, upd_verdict, sizeof(unsigned long long) * 2 * VALIDATE_VERDICT_KEYS, hipMemcpyDeviceToHost, st));
        }
        HIPC(hipStreamSynchronize(st));
        prof.harvest();
        // the verdict, in the order of the host tests of update_matrices_csc: finite (P, then A), symmetric, range
        const unsigned long long *vP = h_verdict, *vA = h_verdict + VALIDATE_VERDICT_KEYS;
        ValuesVerdict verdict;
        if (vP[0] || vA[0]) { verdict.not_finite = vP[0] ? "P" : "A"; return verdict; }
        if (vP[1]) { verdict.asymmetric_column = (int64_t)(~0ull - vP[1]); return verdict; }
        if (eK) {
            auto as_double = [](unsigned long long b) { double d; std::memcpy(&d, &b, sizeof d); return d; };
            const double hi = as_double(std::max(vP[2], vA[2]));
            const unsigned long long lk = std::max(vP[3], vA[3]);
            equil_check_range<T>(hi, lk ? as_double(~0ull - lk) : INFINITY, "qps_update_shared_values");
        }
        {
            ProfScope ps(prof, cat_upd_refresh, 1);
            if (doP) {
                refresh_values<T>(st, upd_src, nullptr, eP, np, const_cast<T*>(P.va));
                values_replaced(false, upd_src, eK, np, location == QPS_MEM_HOST ? Pv : nullptr);
            }
            if (doA) {
                refresh_values<T>(st, upd_src + np, upd_map, eA, na, const_cast<T*>(A.va));
                refresh_values<T>(st, upd_src + np, nullptr, eAt, na, const_cast<T*>(At.va));
                values_replaced(true, upd_src + np, eK ? eK + np : nullptr, na, location == QPS_MEM_HOST ? Av : nullptr);
            }
        }
        HIPC(hipStreamSynchronize(st));
        prof.harvest();
        factor_valid = false;
        this->last_conv.clear();
        return verdict;
    }

  protected:
    // The CSR copy of P is in CSC order (symmetric, full storage) and the rows of A' are the columns of A, so both gradients come out in the canonical order
    // without a map.  adj_rowP / adj_rowAt are built at the first call and kept, like upd_map; the two result arrays live for this call.
    void value_gradients(const T* rx, const T* xv, const T* rl, const T* yv, double* dP, double* dA) override {
        const int64_t np = nnzP(), na = nnzA();
        if (!adj_rowP) {
            const std::vector<int> rP = layout::csc_column_of_entry(n, hPcp), rA = layout::csc_column_of_entry(n, hAcp);
            adj_rowP = mem.template dalloc<int>(np, st); adj_rowAt = mem.template dalloc<int>(na, st);
            if (np > 0) up->copy(adj_rowP, rP.data(), sizeof(int) * (size_t)np);
            if (na > 0) up->copy(adj_rowAt, rA.data(), sizeof(int) * (size_t)na);
            // the two indices and the result per entry, the four panels once
            cat_adj_values = prof.category("shared adjoint: value gradients of P and A", 16.0 * (np + na) + sizeof(T) * 16.0 * npanel * (2.0 * n + 2.0 * m));
        }
        DeviceOwner wm;
        double* d = wm.dalloc<double>(np + na, st);
        {
            ProfScope ps(prof, cat_adj_values, 1);
            if (dP && np > 0) panel_value_gradient<T>(st, np, adj_rowP, P.ci, rx, xv, (int)n, xv, rx, (int)n, npanel, -0.5, d);      // -(r_i x_j + r_j x_i) / 2
            if (dA && na > 0) panel_value_gradient<T>(st, na, adj_rowAt, At.ci, rx, xv, (int)n, yv, rl, (int)m, npanel, -1.0, d + np);   // -(y_i r_j + rl_i x_j)
        }
        if (dP && np > 0) HIPC(hipMemcpyAsync(dP, d, sizeof(double) * (size_t)np, hipMemcpyDeviceToHost, st));
        if (dA && na > 0) HIPC(hipMemcpyAsync(dA, d + np, sizeof(double) * (size_t)na, hipMemcpyDeviceToHost, st));
        HIPC(hipStreamSynchronize(st));
        prof.harvest();
    }
    // QPS_MEM_DEVICE: "device memory, this device" by the pointer attributes, or QPS_ERR_BAD_ARGUMENT.  Host code only; nothing is enqueued.
    void require_device_memory(const char* name, const double* p) const {
        hipPointerAttribute_t at;
        const hipError_t rc = hipPointerGetAttributes(&at, p);
        if (rc != hipSuccess) (void)hipGetLastError();             // an unregistered host pointer is an error of that call on some runtimes: not a sticky one
        if (rc == hipSuccess && at.type == hipMemoryTypeDevice && at.device == device) return;
        throw QpsError(QPS_ERR_BAD_ARGUMENT, std::string("qps_update_shared_values: ") + name + " is not device memory on the handle's device (location = "
                                             "QPS_MEM_DEVICE); the handle is unchanged");
    }
    // cnt doubles into the staging, ordered on the handle's stream: through the uploader, or device to device (the caller's work on them has completed)
    void stage_values(double* dst, const double* src, int64_t cnt, int location) {
        if (location == QPS_MEM_HOST) up->copy(dst, src, sizeof(double) * (size_t)cnt);
        else HIPC(hipMemcpyAsync(dst, src, sizeof(double) * (size_t)cnt, hipMemcpyDeviceToDevice, st));
    }
    // The three hooks of update_matrices_csc and update_values; the CG path leaves them as they are.
    // Before anything is modified, and before any allocation or upload: the path's refusal of the new values (the pattern has been compared)
    virtual void check_new_values(const CanonicalCsc&, const CanonicalCsc&) {}
    // One exponent per entry, on the device, in the order of the value arrays -- the factor's [P; A] in CSC order, then the CSR copies P, A, A' -- or null
    virtual const int* update_exponents() { return nullptr; }
    // The refresh of the CSR copies of P (isA false) or A with `cnt` new values is on the stream: src is their staging on the device in CSC order, e the
    // exponents of that block of the factor's values or null, host the same values in host memory or null (they came from device memory: a path that keeps
    // host copies fetches them from src).  Called for a matrix that was given and has entries.
    virtual void values_replaced(bool /*isA*/, const double* /*src*/, const int* /*e*/, int64_t /*cnt*/, const double* /*host*/) {}
    // what both begin_solve end their clearing with: OSQP's warm_start(x, y) in mode 2, z = A x~ without projection, then the mask
    void start_columns(int warm) {
        if (warm == 2) { ProfScope ps(prof, cat_start, 1); csr_panel<T>(st, A, x, (int)n, z, (int)m, npanel); }
        this->push_active();
    }
    void check_products(const T* xv, const T* yv) override {
        csr_panel<T>(st, A, xv, (int)n, Ax, (int)m, npanel);
        csr_panel<T>(st, P, xv, (int)n, Px, (int)n, npanel);
        csr_panel<T>(st, At, yv, (int)m, Aty, (int)n, npanel);
    }
};

// =================================================================================================================
// Sparse path (a lasso / SVM regularisation path, a scenario sweep on a sparse model).  The linear system is the sparse L D L' of the KKT matrix (k_ldl.hip):
// ordering and symbolic factor once at creation (host only), ONE numeric factorisation per (rho, sigma), and every iteration runs the level-scheduled sweeps on
// 16-column panels -- the index and value of a factor entry are loaded once for 16 QPs, the launch chain is paid once per batch.  The check's A x, P x, A'y are
// CSR x panel products (k_csr_panel.hip).  Panels are n and m rows long, without padding rows.
// =================================================================================================================
template <typename T> struct SparseSharedBatchSolver final : CsrFamilySolver<T> {
    using B = CsrFamilySolver<T>;
    using B::device; using B::n; using B::m; using B::prof; using B::mem; using B::st; using B::up; using B::CP; using B::npanel;
    using B::q; using B::l; using B::u; using B::x; using B::xp; using B::z; using B::zp; using B::y;
    using B::d_active; using B::factor_valid; using B::fac_rho; using B::fac_sigma; using B::num_factorizations;
    using B::cat_chk; using B::cat_fac; using B::cat_switch; using B::cat_start; using B::rho_scale; using B::rs_rho; using B::rs_rho1;
    using B::kd; using B::ke; using B::eq_kd; using B::eq_ke; using B::P; using B::A; using B::At; using B::hPcp; using B::hPri; using B::hAcp; using B::hAri;
    std::unique_ptr<SparseLdl<T>> ldl;   // reads rs_rho / rs_rho1 in its numeric factorisation and panel kernels while a scale is set
    LdlPanelProf pf;
    // Equilibration: the exponents come from the host copy of the canonical CSC arrays (values rounded to T); while it is on, the factor's value array and the
    // three CSR value arrays of the check hold the scaled entries.  Ordering, symbolic factor and every index array stay as they are.
    std::vector<double> hPnz, hAnz;
    // qps_update_shared_matrices_csc while the equilibration is on: the exponent of every entry of the four value arrays, built at the first update under a
    // scaling and kept; it goes whenever the scaling changes
    int* upd_e = nullptr;
    LdlPanelState<T> s; bool rhs_ready = false;   // the running solve

    SparseSharedBatchSolver(int dev, int cnt, int64_t n_, int64_t m_, SparseSharedInput&& in, const double* qh, const double* lh, const double* uh)
        : B(dev, cnt, n_, m_, "a sparse", std::move(in.Pcp), std::move(in.Pri), in.Pnz, std::move(in.Acp), std::move(in.Ari), in.Anz) {
        const int64_t pnnz = this->nnzP(), annz = this->nnzA();
        const int64_t nnzL = (int64_t)in.sym.ci.size(); const int N = in.sym.N, Ns = in.sym.Ns, ldt = in.sym.ldt;
        ldl = make_sparse_ldl<T>(st, std::move(in.sym), in.Pnz.data(), pnnz, in.Anz.data(), annz);
        ldl->panels_prepare(npanel, in.spr);
        hPnz = std::move(in.Pnz); hAnz = std::move(in.Anz);
        this->alloc_state_panels();
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
    // one exponent per entry, in the order of each value array: the factor's [P; A] in CSC order, then the CSR copies P, A, A'
    std::vector<int> entry_exponents(const std::vector<int>& hd, const std::vector<int>& he) const {
        const int64_t pnnz = this->nnzP(), annz = this->nnzA();
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
        const int64_t pnnz = this->nnzP(), annz = this->nnzA();
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
            const int64_t pnnz = this->nnzP(), annz = this->nnzA();
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
    void rho_scale_changed(const double*) override {
        ldl->set_row_rho(rs_rho, rs_rho1);   // both null once the scale is gone
        factor_valid = false;                // the factor belongs to the previous scale
    }
    // the kept exponents on the new values
    void check_new_values(const CanonicalCsc& Pc, const CanonicalCsc& Ac) override {
        if (!kd) return;
        double hi = 0, lo = INFINITY;
        for (int64_t j = 0; j < n; ++j) {
            for (int64_t k = hPcp[j]; Pc.given && k < hPcp[j + 1]; ++k) equil_range_add<T>(Pc.nz[k], eq_kd[hPri[k]] + eq_kd[j], hi, lo);
            for (int64_t k = hAcp[j]; Ac.given && k < hAcp[j + 1]; ++k) equil_range_add<T>(Ac.nz[k], eq_ke[hAri[k]] + eq_kd[j], hi, lo);
        }
        equil_check_range<T>(hi, lo, "qps_update_shared_matrices_csc");
    }
    const int* update_exponents() override {
        if (kd && !upd_e) {
            const std::vector<int> e = entry_exponents(eq_kd, eq_ke);
            upd_e = mem.template dalloc<int>((int64_t)e.size(), st);
            if (!e.empty()) up->copy(upd_e, e.data(), sizeof(int) * e.size());
        }
        return upd_e;
    }
    void values_replaced(bool isA, const double* src, const int* e, int64_t cnt, const double* host) override {
        ldl->set_values(src, e, isA ? this->nnzP() : 0, cnt);
        // what a later qps_set_shared_equilibration computes its exponents from: kept current at every committed update -- device input is copied back here,
        // not fetched when the scaling next asks (the staging is scratch: a refused update in between may have overwritten it)
        std::vector<double>& keep = isA ? hAnz : hPnz;
        if (host) keep.assign(host, host + cnt);
        else HIPC(hipMemcpyAsync(keep.data(), src, sizeof(double) * (size_t)cnt, hipMemcpyDeviceToHost, st));   // complete at the update's closing synchronisation
    }
    void begin_solve(int warm, double, double, double) override {
        this->reset_state(warm);             // from mode 1 on the first right-hand side is built from the z and y that stay (rhs_ready)
        this->start_columns(warm);
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
};

// =================================================================================================================
// Matrix-free CG path (a scenario sweep on a model whose pattern fills in under any ordering).  No factor: every ADMM iteration runs LinOpCg!
// (LinearSystemSolvers.jl:164-186) for all columns in lockstep on 16-column panels (k_cg_panel.hip) -- the indices and values of P, A and A' are read once per
// CG iteration for 16 QPs and the launch chain of an iteration is paid once per batch.  Every column keeps its own cg! scalars on the device; the host reads
// them once per burst of iterations and a column that is done turns into a no-op.  A rho switch costs nothing, the per-row rho scale is a multiplier in the
// epilogue of A u.  Panels are n and m rows long, without padding rows.
// =================================================================================================================
template <typename T> struct CgSharedBatchSolver final : CsrFamilySolver<T> {
    using B = CsrFamilySolver<T>;
    using B::n; using B::m; using B::count; using B::prof; using B::mem; using B::st; using B::CP; using B::npanel;
    using B::q; using B::l; using B::u; using B::x; using B::xp; using B::z; using B::zp; using B::y;
    using B::d_active; using B::active; using B::factor_valid; using B::fac_rho; using B::fac_sigma;
    using B::cat_chk; using B::cat_fac; using B::cat_switch; using B::cat_start; using B::rho_scale; using B::rs_rho; using B::rs_rho1;
    CgPanelArgs<T> a;                      // the matrices (copies of the base's three descriptors), the panels and the scalars of the launches
    T* w = nullptr;
    CgPanelState* h_state = nullptr;       // pinned: [0, CP) the scalars after the last burst, [CP, 2 CP) those cg! started from
    std::vector<int64_t> cg_total;         // per column, over the ADMM iterations of the running solve
    int last_cg = 0; double eps_pcg = 1e-6; int itr_pcg = 1000;
    int cat_rhs = 0, cat_it = 0, cat_post = 0;
    // qps_set_shared_column_rho: rho_b in [0, CP), 1 / rho_b in [CP, 2 CP) (padding columns: 1), allocated at the first solve under the rule.  1 / rho_b is
    // T(1) / T(rho_b), the division of the scalar path: a column that never switches runs the arithmetic of a fixed rho.  With a row scale the rows hold
    // s_i and 1 / s_i (push_row_rho at base 1) and the kernels multiply: two roundings where the scalar path has one.
    T* col_rho = nullptr; std::vector<T> h_col_rho;

    CgSharedBatchSolver(int dev, int cnt, int64_t n_, int64_t m_, CgSharedInput&& in, const double* qh, const double* lh, const double* uh)
        : B(dev, cnt, n_, m_, "a CG", std::move(in.Pcp), std::move(in.Pri), in.Pnz, std::move(in.Acp), std::move(in.Ari), in.Anz) {
        const int64_t pnnz = this->nnzP(), annz = this->nnzA();
        a.n = (int)n; a.m = (int)m; a.npanel = npanel;
        a.P = this->P; a.A = this->A; a.At = this->At;
        a.spr_op = cg_panel_op_spr(pnnz, annz, (int)n);
        this->alloc_state_panels();
        const int64_t pn = (int64_t)CP * n, pm = (int64_t)CP * m;
        a.xx = mem.template dalloc<T>(pn, st); a.r = mem.template dalloc<T>(pn, st); a.u = mem.template dalloc<T>(pn, st); a.c = mem.template dalloc<T>(pn, st);
        a.t = mem.template dalloc<T>(pn, st); a.v = mem.template dalloc<T>(pm, st); a.w = w = mem.template dalloc<T>(pm, st);
        a.part_uc = mem.template dalloc<double>((int64_t)CP * cg_panel_op_blocks((int)n, a.spr_op), st);
        a.part_rr = mem.template dalloc<double>((int64_t)CP * cg_panel_vec_blocks((int)n), st);
        a.state = mem.template dalloc<CgPanelState>(2 * (int64_t)CP, st);
        h_state = mem.template pinned<CgPanelState>(2 * (size_t)CP);
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
    void set_equilibration(int passes) override {
        if (passes > 0) throw QpsError(QPS_ERR_UNSUPPORTED, "CG shared-matrix batch: equilibration is not supported");
    }
    bool takes_column_rho() const override { return true; }   // nothing is factorised: rho is a multiplier in three kernels

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
        this->reset_state(warm);
        HIPC(hipMemsetAsync(a.xx, 0, sizeof(T) * (size_t)CP * (size_t)n, st));                      // LinearSystemSolvers.jl:147: x~ starts from zero at every solve
        this->start_columns(warm);
        cg_total.assign(count, 0);
        last_cg = 0;
        a.eps_pcg = eps_pcg; a.max_it = itr_pcg;
    }
    void switch_rho(double rho, double) override {
        if (!rho_scale.empty()) this->push_row_rho(rho);                                            // the operator and the row update read rho_i
    }
    // one small upload, ordered on the stream: the three kernels read it from the next launch on (the uploader stages the host values before it returns)
    void column_rho_changed(const std::vector<double>& rho_col) override {
        if (!col_rho) { col_rho = mem.template dalloc<T>(2 * (int64_t)CP, st); h_col_rho.assign(2 * (size_t)CP, T(1)); }
        for (int b = 0; b < count; ++b) { h_col_rho[b] = (T)rho_col[b]; h_col_rho[CP + b] = T(1) / h_col_rho[b]; }
        this->up->copy(col_rho, h_col_rho.data(), sizeof(T) * h_col_rho.size());
    }
    void iterate(int lvl, double rho, double sigma, double alpha) override {
        const bool scaled = !rho_scale.empty(), percol = this->column_rho != 0;
        a.rho = (T)rho; a.sigma = (T)sigma; a.alpha = (T)alpha; a.rho_row = scaled ? rs_rho : nullptr; a.rho1_row = scaled ? rs_rho1 : nullptr;
        a.rho_col = percol ? col_rho : nullptr; a.rho1_col = percol ? col_rho + CP : nullptr;
        {
            ProfScope ps(prof, cat_rhs, lvl);
            if (percol) cg_panel_w<T>(st, a, w);                                                    // the same with rho_b (s_i) of the column
            else panel_w<T>(st, z, y, d_active, a.rho_row, a.rho, (int)m, npanel, w);               // LinearSystemSolvers.jl:176
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
    int64_t column_cg_iterations(int b) override { return b < (int)cg_total.size() ? cg_total[b] : 0; }
};

}  // namespace

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
