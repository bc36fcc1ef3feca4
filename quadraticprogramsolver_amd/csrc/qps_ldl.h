// qps_ldl.h -- device-side sparse direct KKT plugin (internal).  Counterpart of the reference's direct plugin pairs
// LaLdlInit/LaLdl!, QDLdlInit/QDLdl!, FacLdlInit/FacLdl! (LinearSystemSolvers.jl:16-107).
#pragma once
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <vector>

#include "ldl_symbolic.h"
#include "qps_internal.h"

namespace qps {

// The ADMM state of a shared-matrix batch in 16-column panels (qps_kernels.h): n-vectors [panel][n][16], m-vectors [panel][m][16], one `active` word per column.
template <typename T> struct LdlPanelState {
    T *x = nullptr, *xp = nullptr; const T* q = nullptr; T *z = nullptr, *zp = nullptr, *y = nullptr; const T *l = nullptr, *u = nullptr;
    const int* active = nullptr; int npanel = 0;
};
// Profiler categories of iterate_panels (prof == nullptr or a level below lvl: no events)
struct LdlPanelProf { Profiler* prof = nullptr; int lvl = 2; int cat_rhs = 0, cat_fwd = 0, cat_tail = 0, cat_bwd = 0, cat_post = 0; };

template <typename T> struct SparseLdl {
    virtual ~SparseLdl() {}
    // numeric L D L' of K(rho, sigma) on the device; symbolic data is reused (the changedRho branch :30-32 / :61-63 / :93-95)
    virtual void factorize(double rho, double sigma) = 0;
    // LinSysSol! body (:37-40): rhs [sigma x - q; z - y / rho], solve in place, xx = x~, zz = z + (nu - y) / rho
    virtual void solve(const T* x, const T* q, const T* z, const T* y, double rho, double sigma, T* xx, T* zz) = 0;
    // One whole ADMM iteration around the solve (SolveQuadraticProgram.jl:54-61): the sweeps, then ONE launch that un-permutes,
    // forms z~ (:40), applies the x / z / y updates (:56-61) and writes the NEXT iteration's permuted right-hand side (:37-38) --
    // two launches fewer per iteration than solve() + admm_update.  rhs_ready: the previous call of iterate() with the same
    // (rho, sigma) already left the right-hand side in place.
    virtual void iterate(T* x, T* xp, const T* q, T* z, T* zp, T* y, const T* l, const T* u, double alpha, double rho, double sigma, bool rhs_ready) = 0;
    // K(rho, sigma) [out_x; out_nu] = [r1; r2] with the factor of the last factorize(): the multiplier block comes back as it is
    // (solve() folds it into z~ = z + (nu - y) / rho, which loses nu when rho is huge)
    virtual void solve_raw(const T* r1, const T* r2, T* out_x, T* out_nu) = 0;
    // Panel forms (shared-matrix batch: many right-hand sides on one factor).  panels_prepare allocates the permuted right-hand side [panel][N][16] and the tail
    // vectors [panel][ldt][16]; spr = 1 | 4 | 16 forces that strip count for every level (0: per level from the mean row length).  iterate_panels is iterate() for
    // every column at once: a column whose active word is 0 keeps its x, xp, z, zp, y.  The summation order of an element depends on the factor's pattern and the
    // strip count only, so a column does not see the batch around it.
    virtual void panels_prepare(int npanel, int spr) = 0;
    virtual void iterate_panels(const LdlPanelState<T>& s, double alpha, double rho, double sigma, bool rhs_ready, const LdlPanelProf& pf) = 0;
    virtual int panel_launches_per_solve() const = 0;
    // rho read as diag(rho_i) (qps_set_shared_rho_scale): device vectors of length m holding rho_i and 1 / rho_i, indexed by the CALLER's row number (the
    // kernels go through perm / iperm); nullptr, nullptr: back to the scalar.  The next factorize() puts -1 / rho_i on the diagonal of constraint row i -- in
    // the sparse levels and in the dense tail alike -- and iterate_panels() reads them in its right-hand side and row updates; both then ignore the scalar rho.
    // solve(), iterate() and solve_raw() of stand-alone handles do not look at them.
    virtual void set_row_rho(const T* rho_row, const T* rho1_row) = 0;
    // Equilibration of the shared-matrix batch (qps_set_shared_equilibration): value k of the factor's input array -- [P values; A values] in the caller's CSC
    // order -- is multiplied by 2^(sign e[k]) in place on the handle's stream (e: device array, one exponent per entry, built by the caller from the pattern).
    // The pattern, the ordering and the symbolic factor stay; the numeric factor is stale until the next factorize().
    virtual void rescale_values(const int* e, int sign) = 0;
    // New values on the frozen pattern (qps_update_shared_matrices_csc): entries [first, first + cnt) of the factor's input array -- P's values from 0, A's from
    // nnz(P), the caller's CSC order -- become 2^e[k] (T) src[k] (src: device doubles, e: device exponents or nullptr), on the handle's stream.  The next
    // factorize() is the pattern-reusing re-factorisation on them; until then the numeric factor is stale.
    virtual void set_values(const double* src, const int* e, int64_t first, int64_t cnt) = 0;
    virtual const LdlSymbolic& symbolic() const = 0;
    virtual int launches_per_solve() const = 0;
    virtual double bytes_per_solve() const = 0;
};

// Pvals / Avals: the caller's CSC value arrays (P full symmetric storage), same order as the index arrays given to ldl_analyze
template <typename T>
std::unique_ptr<SparseLdl<T>> make_sparse_ldl(hipStream_t st, LdlSymbolic&& sym, const double* Pvals, int64_t pnnz, const double* Avals, int64_t annz);

// Canonical 0-based host CSC copies of P (n x n, full symmetric storage) and A (m x n): what the analysis of a KKT factor reads.  Kept until the factor
// that needs them exists, then released.
struct KktHostCsc {
    std::vector<int64_t> Pcp, Pri, Acp, Ari; std::vector<double> Pnz, Anz;
    bool released() const { return Pcp.empty() || Acp.empty(); }
    void release() {
        for (auto* v : {&Pcp, &Pri, &Acp, &Ari}) std::vector<int64_t>().swap(*v);
        std::vector<double>().swap(Pnz); std::vector<double>().swap(Anz);
    }
    // ordering + symbolic analysis of [P + sigma I, A'; A, -I / rho] and the device object on it; a pattern the level-scheduled plugin cannot hold is
    // QPS_ERR_UNSUPPORTED with the analysis' own text
    template <typename T> std::unique_ptr<SparseLdl<T>> make_factor(hipStream_t st, int64_t n, int64_t m, const LdlLimits& lim) const {
        LdlSymbolic sym;
        try { sym = ldl_analyze((int)n, (int)m, Pcp.data(), Pri.data(), Acp.data(), Ari.data(), 0, lim.max_tail, lim.min_level_width, lim.max_levels); }
        catch (const std::runtime_error& e) { throw QpsError(QPS_ERR_UNSUPPORTED, e.what()); }
        return make_sparse_ldl<T>(st, std::move(sym), Pnz.data(), (int64_t)Pnz.size(), Anz.data(), (int64_t)Anz.size());
    }
};

// The direct KKT plugin of a CSC handle (LinearSystemSolvers.jl:16-107): built on first use from the canonical host copies, one numeric factor cached per (rho, sigma)
template <typename T> struct KktPlugin {
    hipStream_t st = nullptr; int64_t n = 0, m = 0;
    KktHostCsc host;
    std::unique_ptr<SparseLdl<T>> ldl; bool valid = false; double rho = 0, sigma = 0;
    int num_factorizations = 0; bool unfit = false;   // unfit: the analysis refused this pattern once (AUTO then goes to CG without asking again)
    KktPlugin(hipStream_t st_, int64_t n_, int64_t m_) : st(st_), n(n_), m(m_) {}
    bool released() const { return host.released(); }   // the host copies went into the factor: a later CG request stays matrix-free (explicit_prepare)
    // LaLdlInit / QDLdlInit / FacLdlInit (LinearSystemSolvers.jl:16-24, :47-55, :78-86): ordering + symbolic once per handle, numeric per (rho, sigma)
    void prepare(double rho_, double sigma_, bool force) {
        if (!ldl) {
            if (n + m > 2000000000LL) throw QpsError(QPS_ERR_BAD_DIMENSION, "KKT matrix too large for the sparse direct plugin");
            // read at every analysis (once per handle), not once per process: the limits are part of a handle's layout
            ldl = host.template make_factor<T>(st, n, m, ldl_limits_from_env());
            valid = false;
            host.release();                                                                         // the canonical host copies have served their purpose
        }
        if (force || !valid || rho != rho_ || sigma != sigma_) {
            valid = false;
            ++num_factorizations;
            ldl->factorize(rho_, sigma_);
            valid = true; rho = rho_; sigma = sigma_;
        }
    }
};

// Dense signed Cholesky M = Lt J Lt' (J = diag(sgn), sgn = +-1 known beforehand: quasi-definite matrices) of an NP x NP row-major
// matrix (lower), in place; dinv receives the inverses of the 64 x 64 diagonal blocks of Lt, W (NP x NP scratch) the panels Lt J.
template <typename T> void cholesky_signed(hipStream_t st, int NP, T* M, T* dinv, int* fail_dev, const T* sgn, T* W);

}  // namespace qps
