// admm_loop.h -- what the single-problem ADMM drivers (DenseSolver, SparseSolver) keep across the iterations of SolveQuadraticProgram.jl:36-73 and report
// alike.  Host only.
#pragma once
#include <cmath>
#include <cstdlib>

#include "qps_polish.h"

namespace qps {

// the rho switch of SolveQuadraticProgram.jl:47
inline bool wants_rho_switch(const qps_params& p, double rho, double rhorho) { return p.adptRho && ((rhorho * p.fctrRho < rho) || (rhorho > p.fctrRho * rho)); }
inline double eps_admm(const qps_params& p) { return std::fmin(p.epsAbs, p.epsRel) * 1e-2; }                                     // :34
inline int iterations_done(int ii, int numIterations) { return ii > numIterations ? numIterations : ii; }   // a loop that ran out stands one past the end
// QPS_GRAPH, read once per process: 0 never replay graphs, another number: wherever the driver can, unset (-1): the driver's own rule
inline int graph_env() { static const int v = [] { const char* e = getenv("QPS_GRAPH"); return e ? atoi(e) : -1; }(); return v; }

struct AdmmLoop {
    double rho, rhorho;                  // the rho in use, the one the last check proposed (:43)
    int convFlag = QPS_CONV_NUM_ITR;     // :33
    double resP = NAN, resD = NAN;
    int nref = 0; double tref = 0;       // rho switches and the seconds their re-factorisations took
    explicit AdmmLoop(double rho0) : rho(rho0), rhorho(rho0) {}
    bool wants_rho_switch(const qps_params& p) const { return qps::wants_rho_switch(p, rho, rhorho); }
    // what check_convergence left in the read-back block
    void read_check(const double* res_host) { resP = res_host[0]; resD = res_host[1]; rhorho = res_host[4]; convFlag = (int)res_host[5]; }
    // the fields every driver fills alike; trsvBlock, sweepVariant, sweepGaveUp, cgIterations and cgExplicit are the driver's own
    void fill_info(qps_info* info, int iterations, double tSetup, double tLoop, const PolishReport& pr) const {
        info->convFlag = convFlag; info->iterations = iterations; info->numRefactor = nref;
        info->rhoFinal = rho; info->rhoProposed = rhorho; info->resPrim = resP; info->resDual = resD;
        info->tSetup = tSetup; info->tLoop = tLoop; info->tRefactor = tref;
        info->polishFlag = pr.flag; info->polishIterations = pr.minresIterations; info->tPolish = pr.seconds;
    }
};

inline void to_c_report(const PolishReport& pr, qps_polish_report* rep) {
    rep->flag = pr.flag; rep->refinements = pr.refinements; rep->minresIterations = pr.minresIterations;
    rep->numActiveLower = pr.numLower; rep->numActiveUpper = pr.numUpper; rep->reserved0 = 0; rep->relres = pr.relres; rep->seconds = pr.seconds;
}

}  // namespace qps
