// shared_family_rules.h -- the two host-side rules of the shared-matrix batches (qps_shared_family.h): the equilibration step and the family-wide rho proposal.
// Plain host arithmetic, no HIP: the CPU suite calls them through tests/capi/layout_shim.cpp and holds them to the numpy restatements of
// tests/equilibration_cases.py and tests/family_rho_cases.py.
#pragma once
#include <cmath>
#include <vector>

namespace qps {

// Ruiz equilibration of the shared-matrix batches with exact powers of two (qps_set_shared_equilibration).  The step for a norm v = f 2^e, f in [0.5, 1), is
// -floor(e / 2): the power of two nearest to 1 / sqrt(v) on a log scale; 0 for v = 0.  Exponents stay in [-13, 13] (OSQP's [1e-4, 1e4]).
constexpr int EQUIL_CLAMP = 13;
inline int equil_step(double v) {
    if (!(v > 0.0)) return 0;
    int e; (void)std::frexp(v, &e);
    return -(int)std::floor(e / 2.0);
}

// Family-wide adaptive rho of the shared-matrix batches (qps_set_shared_adaptive_rho): the proposal of SolveQuadraticProgram.jl:92-96 with the four norms taken from
// the worst columns still running after this check -- bp = argmax normResPrim / maxNormPrim, bd = argmax normResDual / maxNormDual (lowest index on ties, a NaN
// quotient never wins against a number).  res: 8 doubles per column as k_shared_decide leaves them ([0..3] the four norms).  No running column: rhorho stays.
// With one column this is k_check_decide's expression; a NaN proposal stays NaN and never passes the switch test of :47.
inline double family_rho_proposal(const double* res, const std::vector<int>& active, int count, double rho, double rhorho) {
    int bp = -1, bd = -1; double qp = 0, qd = 0;
    for (int b = 0; b < count; ++b) {
        if (!active[b]) continue;
        const double* r = res + 8 * b;
        const double p = r[0] / r[2], d = r[1] / r[3];
        if (bp < 0 || (std::isnan(qp) && !std::isnan(p)) || p > qp) { bp = b; qp = p; }
        if (bd < 0 || (std::isnan(qd) && !std::isnan(d)) || d > qd) { bd = b; qd = d; }
    }
    if (bp < 0) return rhorho;
    const double MIN_VAL_RHO = 1e-3, MAX_VAL_RHO = 1e6;                                     // :81-82
    const double numeratorVal = res[8 * bp + 0] * res[8 * bd + 3];                          // normResPrim_bp * maxNormDual_bd
    const double denominatorVal = res[8 * bd + 1] * res[8 * bp + 2];                        // normResDual_bd * maxNormPrim_bp
    const double t = rho * std::sqrt(numeratorVal / denominatorVal);
    return t > MAX_VAL_RHO ? MAX_VAL_RHO : (t < MIN_VAL_RHO ? MIN_VAL_RHO : t);
}

}  // namespace qps
