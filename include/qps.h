/*
 * qps.h -- C ABI of the MI355X-native ADMM QP solver (libqps_hip.so).
 *
 * Drop-in boundary for ONE path of RoyiAvital/QuadraticProgramSolver (citations are file:line under the
 * reference repository):
 *
 *   SolveQuadraticProgram!(vX, mP, vQ, mA, vL, vU, LinSysSolInit, LinSysSol!; kw...) -> ConvergenceFlag
 *                                                     SolveQuadraticProgram.jl:14-76   -> qps_create_* + qps_solve
 *   CheckConvergence(...)                             SolveQuadraticProgram.jl:79-112  -> inside qps_solve (device)
 *   LinSysSolInit(vX,mP,vQ,mA,rho,rho1,sigma,n,m)     LinearSystemSolvers.jl:16,47,78,110,145 -> qps_linsys_init
 *   LinSysSol!(tuSolver,vXX,vZZ,vX,...,changedRho)    LinearSystemSolvers.jl:28,59,91,125,164 -> qps_linsys_solve
 *   @enum ConvergenceFlag                             SolveQuadraticProgram.jl:12      -> qps_conv_flag
 *   polishing block (MATLAB implementation only)      SolveQuadraticProgram.m:289-325  -> qps_polish, qps_params.polish
 *   ProxQP(mP,vQ,mA,vB,mC,vD[,vX,vY,vZ,vS]) + SolveQuadraticProgram!(sQpProb; kw...) -> dReport
 *                                                     ProxQP.jl:36,73-93,118-173      -> qps_proxqp_*
 *
 * Everything crossing this boundary is a plain pointer, size or scalar.  Host arrays stay owned by the caller and may
 * be freed as soon as the call that received them returns (qps_create_* copies the problem into HBM).
 * A handle is bound to one device and one HIP stream; distinct handles -- on one device or on several devices of the process --
 * may be driven from distinct host threads (per-device state of the library is keyed by device ordinal), a
 * single handle is not thread-safe.  All functions return a qps_status (0 = ok).
 */
#ifndef QPS_H
#define QPS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QPS_VERSION_MAJOR 0
#define QPS_VERSION_MINOR 1

typedef struct qps_solver_s *qps_handle;

typedef enum {
    QPS_OK = 0,
    QPS_ERR_BAD_ARGUMENT = 1,     /* null pointer, negative size, unknown enum value                             */
    QPS_ERR_BAD_DIMENSION = 2,    /* mirrors the dimension checks of SolveQuadraticProgram.m:158-184             */
    QPS_ERR_NOT_FINITE = 3,       /* NaN/Inf in P, q, A or NaN in l/u (l,u may be +-Inf)                         */
    QPS_ERR_FACTORIZATION = 4,    /* Cholesky breakdown (non-positive pivot); qps_last_error names the column    */
    QPS_ERR_HIP = 5,              /* a HIP runtime call failed; qps_last_error carries hipGetErrorString         */
    QPS_ERR_OUT_OF_MEMORY = 6,
    QPS_ERR_NO_DEVICE = 7,        /* no gfx950 device visible: the library never falls back to the CPU           */
    QPS_ERR_UNSUPPORTED = 8
} qps_status;

/* SolveQuadraticProgram.jl:12  @enum ConvergenceFlag convNumItr = 1 convAdmm convPrimDual */
typedef enum {
    QPS_CONV_NUM_ITR = 1, QPS_CONV_ADMM = 2, QPS_CONV_PRIM_DUAL = 3,
    /* additive, issued only by a shared-matrix batch handle with qps_set_shared_infeasibility on */
    QPS_CONV_PRIMAL_INFEASIBLE = 4, QPS_CONV_DUAL_INFEASIBLE = 5
} qps_conv_flag;

/* arithmetic type of the device-resident loop */
typedef enum { QPS_F64 = 0, QPS_F32 = 1 } qps_dtype;

/* which linear-system path replaces the reference plugin pair */
typedef enum {
    QPS_LINSYS_AUTO = 0,        /* dense handle -> QPS_LINSYS_CHOLESKY; CSC handle -> the reference's modeAuto rule on the handle's
                                   sizes (qps_linsys_auto: KKT_LDL or CG), CG when the direct factor does not fit the device plugin */
    QPS_LINSYS_CHOLESKY = 1,    /* reduced form P + sigma I + rho A'A, one Cholesky + two triangular sweeps / it   */
    QPS_LINSYS_CG = 2,          /* matrix-free CG on the reduced operator (LinearSystemSolvers.jl:145-186)         */
    QPS_LINSYS_KKT_LDL = 3,     /* sparse L D L' of the quasi-definite KKT matrix [P + sigma I  A'; A  -I/rho], the reference's
                                   direct plugins LaLdl / QDLdl / FacLdl (LinearSystemSolvers.jl:16-107): minimum-degree ordering
                                   and symbolic factor once per handle, numeric-only re-factorisation on a rho switch, two
                                   level-scheduled sparse triangular solves per iteration.  CSC handles created with dense_path = 0 */
    QPS_LINSYS_CG_EXPLICIT = 4  /* ItrSolCgInit / ItrSolCg! (LinearSystemSolvers.jl:110-142): cg! on the EXPLICIT reduced matrix mL = mPI + rho mAA,
                                   mAA = mA'mA and mPI = mP + sigma I formed once per handle (:112-114), mL rebuilt from the cached parts on a rho switch
                                   (:127-129), ONE product per CG iteration (:137).  CSC handles.  A QPS_LINSYS_CG (or AUTO -> CG) request takes this
                                   plugin by itself when the matrix pays: mA'mA cheap to form and mL no larger than 1.5 x (nnz P + 2 nnz A) -- isotonic
                                   regression, banded / control-like mA; otherwise, and always with QPS_CG_EXPLICIT=0 in the environment, it stays
                                   matrix-free.  Same iterates up to rounding either way (the oracle restates both: linsys kinds 2 and 3) */
} qps_linsys_kind;

/* Keyword arguments of SolveQuadraticProgram! (SolveQuadraticProgram.jl:15-17), same names, same defaults.
 * delta, numItrPolish, epsMinres, numItrMinres are accepted and, exactly as in the reference, unused by the loop; they drive the
 * polishing step of the MATLAB implementation when `polish` is set (see qps_polish below). */
typedef struct {
    int32_t numIterations;   /* 5000 */
    int32_t adptRho;         /* adptΡ, 0/1, default 0 */
    int32_t numItrConv;      /* 25 */
    int32_t numItrPolish;    /* 10; used only when polish != 0 (the Julia loop reserves the kwarg without using it) */
    int32_t numItrMinres;    /* 500; polishing only */
    int32_t linsys;          /* qps_linsys_kind, additive, default AUTO */
    int32_t trsvBlock;       /* additive: size of the inverted diagonal blocks of the blocked triangular sweep; a
                                power-of-two multiple of 64, 0 = library default: one inverted block over the whole factor
                                while the fused forward+backward sweep covers n (n padded <= 16384 fp64 / 32768 fp32), else 4096.
                                1024 or 512 (fp64) / 2048 or 1024 (fp32) with n above it: blocked substitution, ONE launch per
                                sweep (qps_info.sweepVariant = 5); other sizes below n: one launch per block phase (1)         */
    int32_t reuseFactor;     /* additive: 1 = keep the factorisation of a previous qps_solve/linsys_init when
                                (rho, sigma) are unchanged; 0 = factorise on every call like the reference (:36).
                                A dense fp64 handle (single QP, adptRho off, one inverted block; 2048 < n padded <= 4096, or
                                n padded <= 8192 with QPS_WHITEN=1 at creation; QPS_WHITEN=0: never) then iterates in whitened coordinates u = inv(L) t, p = inv(L) x
                                on B = A inv(L)' and G = inv(L) inv(L)', built once per factor inside that solve's tSetup (one
                                more m x n and n x n matrix on the device); x = L p is formed at every check and at the end.
                                Iterates and residuals agree with the classic loop to rounding (1e-12), not bit for bit, and
                                the exact-fixed-point stall test at eps = 0 (|x - xp| <= 0, evaluated as |L (p - pp)|) may fire
                                at a different iteration than in x coordinates                                               */
    double epsAbs;           /* ϵAbs 1e-6 */
    double epsRel;           /* ϵRel 1e-6 */
    double rho;              /* ρ 1 */
    double sigma;            /* σ 1e-6 */
    double alpha;            /* α 1.6 */
    double delta;            /* δ 1e-6; polishing only */
    double fctrRho;          /* fctrΡ 5 */
    double epsMinres;        /* ϵMinres 1e-6; polishing only */
    double epsPcg;           /* CG plugins' ϵPcg 1e-6 (LinearSystemSolvers.jl:125) */
    int32_t numItrPcg;       /* CG plugins' numItrPcg 1000 */
    int32_t loopVariant;     /* additive: 0 = automatic: small problems run the whole loop in one single-workgroup launch,
                                larger ones use the fused single pass over A per iteration when the shape allows (default);
                                1 = unfused kernels (A read twice; the literal order of LinearSystemSolvers.jl:134-139);
                                2 = multi-launch fused loop even for small problems */
    int32_t polish;          /* additive: 0 = no polishing (what SolveQuadraticProgram.jl does, default); 1 = run the polishing step
                                of SolveQuadraticProgram.m:289-325 after the loop with numItrPolish, delta, epsMinres, numItrMinres */
    int32_t reserved0;
} qps_params;

/* Additive out-of-band report (the reference returns only the flag, SolveQuadraticProgram.jl:73). */
typedef struct {
    int32_t convFlag;        /* qps_conv_flag */
    int32_t iterations;      /* loop bodies executed */
    int32_t numRefactor;     /* changedΡ events (each one re-factorises) */
    int32_t cgIterations;    /* total inner CG iterations (QPS_LINSYS_CG) */
    double rhoFinal;         /* ρ in force at exit */
    double rhoProposed;      /* ρρ at exit */
    double resPrim;          /* ||A x - z||_inf at the last check (:85) */
    double resDual;          /* ||P x + q + A'y||_inf at the last check (:86) */
    double tSetup;           /* seconds: LinSysSolInit (assembly + factorisation), device time incl. sync */
    double tLoop;            /* seconds: the iteration loop, device time incl. sync */
    double tRefactor;        /* seconds spent in changedΡ re-factorisations (part of tLoop) */
    int32_t polishFlag;      /* minresFlag of SolveQuadraticProgram.m:311-325: -1 polishing did not run, 0 converged (x replaced),
                                1 the last MINRES call did not converge (x kept) */
    int32_t polishIterations;/* total MINRES iterations of the polishing step */
    double tPolish;          /* seconds spent polishing (not part of tLoop) */
    int32_t trsvBlock;       /* dense handles: size of the inverted diagonal blocks the triangular sweeps ran with (0: not a dense Cholesky run) */
    int32_t sweepVariant;    /* dense handles: 1 = blocked substitution over the sweep matrix (2 n / trsvBlock - 1 dependent phases per sweep),
                                2 = explicit inverse, both sweeps fused into one pass over the triangle (trsvBlock >= n),
                                3 = explicit inverse, two triangular GEMVs, 4 = single-launch small-problem loop,
                                5 = blocked substitution, ONE launch per sweep (n / trsvBlock dependent phases handed from workgroup to
                                    workgroup inside the launch; trsvBlock = 1024 or 512 fp64, 2048 or 1024 fp32); 0 otherwise */
    int32_t sweepGaveUp;     /* times a variant-5 launch of this solve gave up waiting for its workgroups (any concurrent work on the card
                                can cause that, other streams of this process included) and the solve was repeated on variant 1; its time is in
                                tLoop.  A variant-5 solve is bit-reproducible only when this is 0 */
    int32_t cgExplicit;      /* CSC handles, CG plugins: 1 = the solve ran cg! on the explicit reduced matrix (ItrSolCg, one product per CG iteration),
                                0 = on the matrix-free operator (LinOpCg / LinMapsCg) or no CG at all */
} qps_info;

/* Fill *p with the reference defaults (SolveQuadraticProgram.jl:15-17). */
int32_t qps_default_params(qps_params *p);

/* Number of HIP devices visible (0 when there is none; never an error). */
int32_t qps_device_count(void);

/* Dense problem, column-major (Julia Matrix{Float64}): P is n x n (leading dimension ldp), A is m x n (lda).
 * Replaces the data half of the call SolveQuadraticProgram.jl:14 for dense inputs. */
int32_t qps_create_dense(int64_t n, int64_t m, const double *P, int64_t ldp, const double *A, int64_t lda,
                         const double *q, const double *l, const double *u, int32_t dtype, int32_t device,
                         qps_handle *out);

/* Sparse problem, CSC (Julia SparseMatrixCSC{Float64,Int64}: colptr, rowval, nzval), index_base 1 for Julia, 0 for C.
 * P must hold the full symmetric matrix (as GenerateQuadraticProgram.jl produces).  dense_path != 0 densifies the
 * problem on the device and uses the Cholesky path; 0 keeps CSR storage and uses the CG path. */
int32_t qps_create_csc(int64_t n, int64_t m,
                       const int64_t *P_colptr, const int64_t *P_rowval, const double *P_nzval,
                       const int64_t *A_colptr, const int64_t *A_rowval, const double *A_nzval,
                       const double *q, const double *l, const double *u, int32_t index_base, int32_t dense_path,
                       int32_t dtype, int32_t device, qps_handle *out);

/* SolveQuadraticProgram! (SolveQuadraticProgram.jl:14-76): x_inout is vX (warm start in, solution out, length n);
 * z and y restart at 0 (:39-40).  info may be NULL.  Blocks until the result is in x_inout. */
int32_t qps_solve(qps_handle h, double *x_inout, const qps_params *params, qps_info *info);

/* The polishing step alone (SolveQuadraticProgram.m:289-325; MATLAB only -- the Julia loop reserves its kwargs,
 * SolveQuadraticProgram.jl:16-17): active sets from the sign of the multiplier y (length m), reduced KKT system, iterative
 * refinement with MINRES (numItrPolish, delta, epsMinres, numItrMinres of *params).  x_inout (length n) is replaced by the
 * polished primal only when report->flag == 0.  Dense and CSR handles (batch handles: through qps_params.polish). */
typedef struct {
    int32_t flag;              /* minresFlag: -1 did not run (numItrPolish <= 0), 0 converged, 1 not converged (x kept) */
    int32_t refinements;       /* bodies of the refinement loop executed (<= numItrPolish) */
    int32_t minresIterations;  /* total MINRES iterations */
    int32_t numActiveLower;    /* numL = sum(vY < 0) */
    int32_t numActiveUpper;    /* numU = sum(vY > 0) */
    int32_t reserved0;
    double relres;             /* ||r|| / ||b|| of the last MINRES call */
    double seconds;
} qps_polish_report;
int32_t qps_polish(qps_handle h, double *x_inout, const double *y, const qps_params *params, qps_polish_report *report);

/* Final z and y of the last qps_solve (length m each; batch handles: [count][m] each, of the last qps_solve_batch; either pointer
 * may be NULL). Additive. */
int32_t qps_get_dual(qps_handle h, double *z_out, double *y_out);

/* The reference plugin pair, literally (host vectors in, device solve, host vectors out):
 *   qps_linsys_init  == LinSysSolInit(vX, mP, vQ, mA, rho, 1/rho, sigma, n, m)       LinearSystemSolvers.jl:110-122
 *   qps_linsys_solve == LinSysSol!(tuSolver, vXX, vZZ, vX, ..., vZ, vY, rho, 1/rho, sigma, n, m, changedRho)  :125-142
 * Post-condition as in the reference: xx_out == x-tilde (n), zz_out == z-tilde (m). */
int32_t qps_linsys_init(qps_handle h, double rho, double sigma, int32_t linsys, int32_t trsvBlock);
int32_t qps_linsys_solve(qps_handle h, const double *x, const double *z, const double *y, double rho, double sigma,
                         int32_t changed_rho, double *xx_out, double *zz_out);
/* The keyword arguments of the CG plugins' Sol!  --  ItrSolCg! / LinOpCg! / LinMapsCg!(...; ϵPcg = 1e-6, numItrPcg = 1000)
 * (LinearSystemSolvers.jl:125, :164, :207): inner tolerance (abstol of IterativeSolvers.cg!) and iteration cap used by the following
 * qps_linsys_solve calls of a CG handle.  Accepted and without effect on the direct plugins (they have no inner iteration). */
int32_t qps_linsys_set_cg(qps_handle h, double epsPcg, int32_t numItrPcg);

/* ONE application of the matrices behind the reduced operator of the CG plugins -- LinOpCgInit / LinMapsCgInit build it from three products,
 *     mul!(vZZ, mA, vW); mul!(vU, mA', vZZ); mul!(vU, mP, vW, 1.0, rho); vU .+= sigma .* vW          LinearSystemSolvers.jl:152-157, :195-200
 * and CheckConvergence applies the same three matrices to x and y (SolveQuadraticProgram.jl:85-89) -- through the device kernels qps_solve itself
 * uses for them on this handle (CSC handles: the column-blocked SpMV when the handle built one, else the CSR-stream kernel; dense handles: the
 * row / column GEMVs).  Host vector in, host vector out, in the handle's arithmetic type on the device:
 *     QPS_OP_P        out[n]     = mP  * in[n]
 *     QPS_OP_A        out[m]     = mA  * in[n]
 *     QPS_OP_AT       out[n]     = mA' * in[m]
 *     QPS_OP_PA       out[n + m] = [mP; mA] * in[n]   (the stacked product of a CG iteration: one pass over `in`)
 *     QPS_OP_REDUCED  out[n]     = mP in + rho mA'(mA in) + sigma in                                    (:152-157; rho, sigma used by this one only)
 * Additive (the reference has no such call): it lets a binding or a test compare the device copies of its matrices with its own product, one
 * operator at a time.  The solver state (x, z, y of the last solve) is not touched. */
typedef enum { QPS_OP_P = 0, QPS_OP_A = 1, QPS_OP_AT = 2, QPS_OP_PA = 3, QPS_OP_REDUCED = 4 } qps_operator_kind;
int32_t qps_operator_apply(qps_handle h, int32_t op, const double *in, double *out, double rho, double sigma);

/* Batch of `count` independent dense QPs of identical shape (BASELINE config 4).  Problem b uses
 * P + b*ldp*n ... i.e. arrays are stacked along a leading batch axis: P[count][n*n], A[count][m*n] (column-major
 * each), q[count][n], l/u[count][m].  x_inout is [count][n]; infos (may be NULL) is [count]. */
int32_t qps_create_dense_batch(int64_t count, int64_t n, int64_t m, const double *P, const double *A, const double *q,
                               const double *l, const double *u, int32_t dtype, int32_t device, qps_handle *out);
int32_t qps_solve_batch(qps_handle h, double *x_inout, const qps_params *params, qps_info *infos);

/* Shared-matrix batch: `count` QPs on ONE P (n x n, ldp) and ONE A (m x n, lda), both column-major as for qps_create_dense, that differ in
 * q [count][n], l [count][m] and u [count][m] only -- an MPC horizon re-solved every sample, a regularisation path, a scenario sweep.  The
 * matrices are stored, factorised and streamed once for all columns.  The handle is a batch handle: qps_solve_batch (x_inout [count][n], infos
 * [count]), qps_get_dual ([count][m]), qps_set_profiling, qps_kernel_times, qps_last_error and qps_destroy work on it, and column b behaves as
 * a stand-alone qps_solve on (P, q_b, A, l_b, u_b): its own check every numItrConv iterations, its own flag, iteration count and residuals,
 * x = the iterate at its own stopping iteration.  Arguments are validated as by qps_create_dense, for every column, before a device is needed.
 * count is limited to 65535, as for qps_create_dense_batch (QPS_ERR_BAD_DIMENSION beyond).
 * QPS_ERR_UNSUPPORTED (qps_last_error names the reason): m = 0 or n padded beyond 16384 (fp64) / 32768 (fp32) at creation; adptRho != 0 (one
 * factor needs one rho), polish != 0 or a trsvBlock other than 0 or >= n at qps_solve_batch -- the handle stays usable afterwards
 * (qps_params.polish stays refused; qps_polish_shared / qps_set_shared_polish run the step).
 * qps_update_shared_vectors replaces q, l and / or u of every column (a NULL pointer keeps the array); the factorisation does not depend on
 * them, so a following qps_solve_batch with reuseFactor = 1 and unchanged (rho, sigma) does not factorise again. */
int32_t qps_create_dense_shared_batch(int64_t count, int64_t n, int64_t m, const double *P, int64_t ldp, const double *A, int64_t lda,
                                      const double *q, const double *l, const double *u, int32_t dtype, int32_t device, qps_handle *out);
int32_t qps_update_shared_vectors(qps_handle h, const double *q, const double *l, const double *u);

/* Per-constraint rho scale of a shared-matrix batch handle (dense or sparse; section 5.2 of the OSQP paper): `scale` is [m], finite and strictly positive, and is
 * shared by all columns -- which rows are equalities is a property of the family.  Row i then runs with rho_i = rho * scale[i], i.e. the loop of
 * SolveQuadraticProgram.jl:54-61 with rho read as diag(rho_i): (P + sigma I + A' diag(rho_i) A) x~ = sigma x - q + A'(rho_i z_i - y_i) (dense handle) or the KKT
 * system with -1 / rho_i on the diagonal of constraint row i (sparse handle), z_i = clamp(alpha z~_i + (1 - alpha) z_i + y_i / rho_i, l_i, u_i),
 * y_i += rho_i (alpha z~_i + (1 - alpha) z_i - z_i_new).  CheckConvergence is unchanged (none of its norms involves rho); qps_params.rho stays the base value and
 * rhoFinal / rhoProposed keep reporting it; every column keeps its own check, flag and stopping iteration; adptRho stays refused.  rho_i and 1 / rho_i are formed in
 * double on the host and rounded once to the handle's type.  One factorisation still serves every column.
 * The vector is copied (the caller may free it on return).  scale = NULL goes back to the scalar rho and releases what the scale needed on the device (dense handle:
 * one more m x n matrix, diag(sqrt(scale)) A, from which A' diag(scale) A is formed as a symmetric product, and three vectors of length m; sparse handle: two).
 * Setting or clearing a scale invalidates the factorisation: the next qps_solve_batch factorises even with reuseFactor = 1; after that reuseFactor and
 * qps_update_shared_vectors behave as before.
 * QPS_ERR_BAD_ARGUMENT: a NULL handle, or an entry that is NaN, Inf, zero or negative (checked before a device is needed; the handle keeps its previous scale and
 * factor).  QPS_ERR_UNSUPPORTED (qps_last_error names the reason): any handle that is not a shared-matrix batch. */
int32_t qps_set_shared_rho_scale(qps_handle h, const double *scale /* [m]; NULL = back to the scalar rho */);

/* Family-wide adaptive rho of a shared-matrix batch handle (dense or sparse).  mode 0 (the default): the fixed rho of qps_params.rho.  mode 1: ONE rho that moves
 * for the whole family by the reference's own rule (SolveQuadraticProgram.jl:92-96 and :47) with the four norms taken from the worst columns.  At a check, after
 * the per-column decisions (unchanged), over the columns still running: bp = argmax normResPrim_b / maxNormPrim_b, bd = argmax normResDual_b / maxNormDual_b
 * (lowest column on ties; a NaN quotient never wins against a number), and
 *   rhoProposed = clamp(rho * sqrt((normResPrim_bp * maxNormDual_bd) / (normResDual_bd * maxNormPrim_bp)), 1e-3, 1e6);
 * no running column leaves it alone.  At the top of the next iteration, rhoProposed * fctrRho < rho || rhoProposed > fctrRho * rho makes rho = rhoProposed: one
 * numeric re-factorisation for the whole batch (dense: assembly from the cached A'A plus Cholesky; sparse: numeric L D L' on the frozen pattern), and every
 * running column continues on the new factor.  With count = 1 this is the adptRho = 1 loop of a stand-alone handle, expression for expression.  The decision is
 * taken on the host from the norms it reads at every check anyway.  qps_params.fctrRho of the solve is used (QPS_ERR_BAD_ARGUMENT unless > 0); qps_params.adptRho
 * names the per-problem rule and stays refused.  With a rho scale set the base rho moves and row i runs with rho * scale[i].
 * qps_info per column: numRefactor = switches while the column was running, rhoFinal = the rho of its last iteration, rhoProposed = the family proposal after the
 * check at which it stopped (or at exit), tRefactor = seconds spent in switches (whole batch, like tLoop).
 * The mode is a property of the handle and persists across solves.  After a solve the factor belongs to the last rho: reuseFactor = 1 with qps_params.rho =
 * rhoFinal of the column that ran longest factorises nothing -- the re-solve pattern after qps_update_shared_vectors.
 * QPS_ERR_BAD_ARGUMENT: a NULL handle or any other mode (before a device is needed).  QPS_ERR_UNSUPPORTED (qps_last_error names the reason): any handle that is
 * not a shared-matrix batch. */
int32_t qps_set_shared_adaptive_rho(qps_handle h, int32_t mode /* 0 fixed rho, 1 family-wide rule */);

/* Per-column adaptive rho of a matrix-free CG shared-matrix batch handle (qps_create_csc_shared_batch_cg), opt-in: the reference's own per-problem rule
 * (SolveQuadraticProgram.jl:43, :47, :92-96) for every column.  Nothing is factorised on that handle and rho enters three kernels as a multiplier, so every
 * column can carry a rho of its own: rho_b = qps_params.rho at the start of every solve (warm start modes do not carry rho across solves); at a check
 * rhorho_b = clamp(rho_b sqrt(normResPrim_b maxNormDual_b / (normResDual_b maxNormPrim_b)), 1e-3, 1e6) from the column's own four norms; at the top of the
 * next iteration rhorho_b fctrRho < rho_b || rhorho_b > fctrRho rho_b makes rho_b = rhorho_b.  A NaN proposal never switches, a column that has stopped keeps its
 * rho, and a column's CG continues from its x~ across a switch.  Column b then equals a stand-alone CSC handle with QPS_LINSYS_CG, matrix-free, adptRho = 1.
 * With a per-row rho scale row i of column b runs on rho_b s_i.  qps_info per column: numRefactor = its own switches, rhoFinal = its rho, rhoProposed = its
 * last proposal.  The batch runs until its slowest column: the gain is per column.  The option is a property of the handle, survives
 * qps_update_shared_matrices_csc and excludes the family rule: turning one on while the other is on is QPS_ERR_UNSUPPORTED (turn the other off first; the
 * handle stays as it was), turning either off is always accepted.  While it is on, qps_solve_batch wants fctrRho > 0 (QPS_ERR_BAD_ARGUMENT); adptRho = 1 in
 * qps_params stays refused.
 * QPS_ERR_BAD_ARGUMENT: a NULL handle, `on` outside {0, 1} (before a device is needed).  QPS_ERR_UNSUPPORTED (qps_last_error names the reason): a handle that is
 * not a shared-matrix batch; on = 1 on a dense or a sparse L D L' shared-matrix batch, where one factor serves every column (they have
 * qps_set_shared_adaptive_rho). */
int32_t qps_set_shared_column_rho(qps_handle h, int32_t on /* 0 = off (default); 1 = every column moves its own rho */);

/* Ruiz equilibration of a shared-matrix batch handle (dense or sparse; section 5.1 of the OSQP paper, item 2 of the reference's to-do list), opt-in: passes = 0
 * (the default) leaves the handle exactly as it is, passes = 1..50 runs that many passes.  The scaling D = diag(2^kd) of the variables and E = diag(2^ke) of the
 * constraints depends on P and A only, so it is computed once for the family and serves every column and every re-solve after qps_update_shared_vectors.  D and E
 * are exact powers of two: scaling and unscaling never round, the exponents are integer arithmetic (the device and a numpy restatement agree exactly), and clearing
 * the option restores the matrices bit for bit -- no second copy of a matrix is kept.
 * The rule: kd = ke = 0; one pass is Jacobi, with all norms taken through the exponents from before the pass,
 *   cn_j = max(max_i |P_ij| 2^(kd_i + kd_j), max_i |A_ij| 2^(ke_i + kd_j)),   rn_i = max_j |A_ij| 2^(ke_i + kd_j),
 * formed in double from the entries as stored in the handle's type (an fp32 handle scales the fp32-rounded matrices).  For a norm v = f 2^e > 0, f in [0.5, 1), the
 * step is -floor(e / 2) -- the power of two nearest to 1 / sqrt(v) on a log scale -- and 0 for v = 0 (an empty row or column); then kd_j = clamp(kd_j + step(cn_j),
 * -13, 13), likewise ke (OSQP's [1e-4, 1e4]).  OSQP's cost scaling c is not applied: it depends on q, which differs per column, and it would scale P.
 * The loop then runs unchanged on D P D, E A D, D q, E l, E u; in the caller's variables that is the ADMM loop with sigma_j = sigma / D_j^2 and rho_i = rho E_i^2,
 * so the iterates differ from those of an unscaled solve.  The warm start goes in as D^-1 x, the result comes back as D x~, qps_get_dual returns E^-1 z~ and E y~, and
 * the convergence check -- hence resPrim / resDual, the per-column flags and the family-wide rho rule -- sees the unscaled norms, as in OSQP.  With a rho scale set,
 * row i runs with rho * scale[i] on the scaled rows.  adptRho and qps_params.polish stay refused; qps_polish_shared / qps_set_shared_polish run the polishing step
 * on the scaled data.
 * Range: after the passes and before anything is modified, the largest and the smallest non-zero scaled matrix magnitude have to be normal numbers of the handle's
 * type (this matters for fp32); otherwise QPS_ERR_UNSUPPORTED and the handle stays as it was.  Vector entries are not range-checked: a scaled bound that overflows
 * is a bound at infinity.
 * Setting, changing or clearing invalidates the factorisation: the next qps_solve_batch factorises even with reuseFactor = 1.  While the option is on the handle
 * keeps two int vectors (n and m) on the device.
 * QPS_ERR_BAD_ARGUMENT: a NULL handle or passes outside 0..50 (before a device is needed; the handle keeps its state).  QPS_ERR_UNSUPPORTED (qps_last_error names
 * the reason): any handle that is not a shared-matrix batch, or the range check above.
 * qps_get_shared_equilibration writes D ([n]) and E ([m]) as doubles, all ones while the option is off; either pointer may be NULL. */
int32_t qps_set_shared_equilibration(qps_handle h, int32_t passes /* 0 = off (default); 1..50 = that many Ruiz passes */);
int32_t qps_get_shared_equilibration(qps_handle h, double *d_out /* [n] or NULL */, double *e_out /* [m] or NULL */);

/* Warm start of z and y across the re-solves of a shared-matrix batch handle (dense or sparse; the OSQP paper warm-starts (x, y) and continues from (x, z, y)),
 * opt-in.  The handle keeps z and y of every column between calls; both are zero from creation on.  mode is a property of the handle and persists across solves:
 *   0 (the default): qps_solve_batch restarts z and y at 0 (SolveQuadraticProgram.jl:39-40); x alone comes from x_inout.
 *   1 ("state"): every column starts from the z and y the handle holds -- the iterates at the column's own stopping iteration of the last qps_solve_batch, or what
 *      qps_set_shared_dual wrote since -- and from the x of x_inout.  On a fresh handle this is the cold start, bit for bit.
 *   2 ("Ax", OSQP's warm_start(x, y)): y comes from the handle and z = A x is formed on the device from the x_inout of this solve, without projection.
 * In modes 1 and 2 xp and zp start at 0 (iteration 1 overwrites them before a check reads them), the iteration counter restarts at 1 -- checks fall on multiples
 * of numItrConv of this solve -- and flags, iterations, residuals, reuseFactor, the family-wide rho rule and qps_info keep their meaning.  A stored z outside new
 * bounds is legal: iteration 1 clamps it.  z and y do not depend on rho: setting or clearing a rho scale or changing qps_params.rho leaves them alone (the dense
 * handle re-forms rho_i z - y for the rho of the solve in one launch), and a change of the equilibration carries them over in the caller's units.  Together with
 * qps_update_shared_vectors and reuseFactor = 1 a re-solve then neither factorises nor starts its iterations over.
 * qps_set_shared_dual is the counterpart of qps_get_dual: z and / or y, [count][m] each in the caller's units (with equilibration on the handle stores E z and
 * E^-1 y: exact powers of two, so writing back what qps_get_dual returned changes no bit, for fp64 and fp32 handles alike).  The arrays are copied; a NULL
 * pointer keeps that array.
 * After a qps_solve_batch that returned an error the stored z and y are unspecified until qps_set_shared_dual or a mode-0 solve.
 * QPS_ERR_BAD_ARGUMENT: a NULL handle, a mode outside 0..2 (judged before the kind of handle), or a NaN / Inf entry of z or y (before a device is needed; the
 * handle keeps its state).  QPS_ERR_UNSUPPORTED (qps_last_error names the reason): any handle that is not a shared-matrix batch.
 * Out of scope: stand-alone handles, qps_create_dense_batch, ProxQP handles (qps_proxqp_set_state serves them). */
int32_t qps_set_shared_warm_start(qps_handle h, int32_t mode /* 0 z = y = 0 (default), 1 the stored z and y, 2 z = A x and the stored y */);
int32_t qps_set_shared_dual(qps_handle h, const double *z, const double *y);   /* [count][m] each; NULL keeps that array */

/* Per-column infeasibility certificates of a shared-matrix batch handle (dense or sparse; section 3.4 of the OSQP paper), opt-in.  Without it a column that has no
 * solution can only end with flag 1 at numIterations: the whole batch pays its launch chain to the end, under qps_set_shared_adaptive_rho it steers the family rho
 * for everyone, and the caller cannot tell "needs more iterations" from "has no solution".  With it such a column stops at a check with a flag of its own and a
 * certificate.  Nothing in the iteration changes; all of the work happens at the checks.
 * The rule, per column, at a check (every numItrConv iterations), in the caller's units.  A column is examined only if it is still running and CheckConvergence
 * leaves its flag at 1 at this check: flags 2 and 3 are decided as before and win.  dx = x - xp and dy = y - y_prev, y_prev being y before this iteration's row
 * update; both differences are formed in the handle's type.
 *   Primal infeasible (QPS_CONV_PRIMAL_INFEASIBLE = 4): dyh = dy projected onto the polar of the recession cone of [l, u] -- dyh_i = 0 if l_i = -Inf and u_i = +Inf,
 *   min(dy_i, 0) if only u_i = +Inf, max(dy_i, 0) if only l_i = -Inf, dy_i otherwise.  With N = ||dyh||_inf and S = sum_{dyh_i > 0} u_i dyh_i + sum_{dyh_i < 0}
 *   l_i dyh_i (entries with dyh_i = 0 are skipped: 0 * Inf never arises), the column is primal infeasible iff
 *       N > epsPrimInf   and   S < -epsPrimInf N   and   ||A'dyh||_inf < epsPrimInf N.
 *   Dual infeasible (QPS_CONV_DUAL_INFEASIBLE = 5), tested only if the primal test failed: with M = ||dx||_inf, iff
 *       M > epsDualInf   and   q'dx < -epsDualInf M   and   ||P dx||_inf < epsDualInf M   and for every row i:
 *       u_i finite implies (A dx)_i < epsDualInf M,   l_i finite implies (A dx)_i > -epsDualInf M.
 *   Every comparison with a NaN operand is false: no certificate.  The norms are inf-norms; the two sums are formed and added in double whatever the handle's type,
 *   in an order that depends on n and m only -- a column of a batch stays bit-identical to the same data in a batch of one, certificate included.
 * A column that gets flag 4 or 5 stops like any other: it is frozen by the active mask, qps_info.iterations is this check's iteration, x, z, y (qps_get_dual) are
 * the iterates of that iteration, resPrim / resDual those of that check, and it leaves the "columns still running" of the family-wide rho rule.
 * epsPrimInf = epsDualInf = 0 (the default) turns the option off: the handle behaves exactly as without it, bit for bit.  A positive finite value turns that test
 * on; one of the two may be 0 to leave that test off.  OSQP's default for each is 1e-4.  The setting is a property of the handle and persists across solves; it does
 * not touch the factorisation, the stored z and y, or reuseFactor.  With it on and every column feasible the results equal those with it off, bit for bit.
 * Interactions.  Rho scale: it does not enter the rule.  Family-wide rho: a switch happens at the top of an iteration, so dy spans one iteration at one rho.
 * Equilibration: the rule sees the caller's units, as the convergence check does -- dy = E dy~, dx = D dx~, A'dyh = D^-1 A~'dyh~, P dx = D^-1 P~ dx~, A dx = E^-1 A~
 * dx~, all moves exact powers of two; the two sums do not change under the scaling.  Warm-start modes 1 and 2: unchanged (xp and y_prev are defined at the first check).
 * Cost: per check one copy of the y panels, two small launches and the check's three matrix products once more, on the differences; the flags travel in the
 * read-back the check makes anyway (still one device-to-host copy and one stream synchronisation per check).  While the option is on the handle holds three more
 * panel arrays ([count][m] twice, [count][n] once) and a small reduction buffer; they are released when it is turned off.
 * fp32 handles: dy is a difference of fp32 iterates, so its absolute error is half an ulp of y, and y of an infeasible column grows with every iteration; ||A'dyh|| /
 * ||dyh|| then stops falling around 1e-4 .. 1e-3 (measured: 2e-4 at n = 96, m = 160).  Give an fp32 handle 1e-3; at 1e-4 such a column may never be flagged.
 * qps_get_shared_certificate: row b of dy ([count][m]) is dyh of column b if its last qps_solve_batch ended with flag 4, else zeros; row b of dx ([count][n]) is dx
 * if it ended with flag 5, else zeros -- both of the column's own stopping check, in the caller's units, unnormalised.  Either pointer may be NULL.  Zeros before any
 * solve, after a solve that returned an error, after the option was turned off and after a change of the equilibration.
 * QPS_ERR_BAD_ARGUMENT: a NULL handle, or a negative, NaN or Inf value (before a device is needed; the handle keeps its state).  QPS_ERR_UNSUPPORTED
 * (qps_last_error names the reason): any handle that is not a shared-matrix batch.
 * Out of scope: stand-alone handles, qps_create_dense_batch, qps_solve_batch_multi, ProxQP handles and the CG plugins. */
int32_t qps_set_shared_infeasibility(qps_handle h, double epsPrimInf, double epsDualInf);   /* 0, 0 = off (default); OSQP: 1e-4, 1e-4 */
int32_t qps_get_shared_certificate(qps_handle h, double *dy /* [count][m] or NULL */, double *dx /* [count][n] or NULL */);

/* Polishing on a shared-matrix batch handle (dense or sparse), opt-in.  qps_params.polish stays refused on these handles; the two entry points below run the step.
 * Per column it is the step of qps_polish: active sets from the sign of y, g = [-q; l(L); u(U)], iterative refinement of K t = g with MINRES on K + blkdiag(delta I,
 * -delta I), x = t(1:n) only where the column's last MINRES call converged.  All columns advance in lockstep on 16-column panels, so P, A and A' are read once per
 * MINRES iteration for 16..32 columns; every column has its own MINRES state, stops on its own residual and is frozen from then on.  In refinement round jj the
 * columns still refining run MINRES together; a column whose call ended with flag 1 leaves with its x kept, the others add the correction and go on.  Inner
 * products are added in an order that depends on n and m only: a column of a batch equals the same data in a batch of one bit for bit, report included.
 * qps_polish_shared uses numItrPolish, delta, epsMinres and numItrMinres of *params and nothing else of it.  It works before any solve, ignores rho, the rho scale,
 * the family rule, the warm-start mode and the certificate setting, and leaves the stored z and y, the factor and everything else the handle keeps untouched: a
 * following qps_solve_batch, warm-started or not, is bit for bit what it would have been.  y = NULL takes the y the handle holds (the last qps_solve_batch or
 * qps_set_shared_dual; zero on a fresh handle: every mask is empty and the system is P t = -q).  reports [count]: flag, refinements, minresIterations, relres,
 * numActiveLower and numActiveUpper are per column, seconds is the wall time of the whole batch's step.
 * qps_set_shared_polish(h, 1): every qps_solve_batch ends with that step on its own x and y, on every column whose flag is not QPS_CONV_PRIMAL_INFEASIBLE or
 * QPS_CONV_DUAL_INFEASIBLE (those keep polishFlag = -1 and their x); polishFlag, polishIterations and tPolish of each qps_info are filled (tPolish: wall time of the
 * whole batch's step, not part of tLoop), the stored z and y stay those of the loop, and x_inout is what qps_polish_shared(h, x, NULL, params, ...) would have made
 * of the unpolished result, bit for bit.  0 (the default): as without it, polishFlag = -1, polishIterations = 0, tPolish = 0.  The switch stays with the handle.
 * Equilibration: the step runs on the scaled data the handle holds, as OSQP's does -- x~ = D^-1 x and y~ = E^-1 y go in, x = D t~_x comes out, all exact powers of
 * two -- so delta regularises, and epsMinres bounds the residual of, the system in the scaled variables.  The active sets do not change (the scaling is positive).
 * QPS_ERR_BAD_ARGUMENT: a NULL handle, x_inout or params, a NaN / Inf in x or y, a delta that is not finite, a NaN epsMinres, an `on` other than 0 or 1 (before
 * a device is needed; the handle is unchanged).  QPS_ERR_UNSUPPORTED (qps_last_error names the reason): any handle that is not a shared-matrix batch.
 * Out of scope: qps_solve_batch_multi, ProxQP handles, a per-column delta, a preconditioner. */
int32_t qps_polish_shared(qps_handle h, double *x_inout, const double *y, const qps_params *params, qps_polish_report *reports);
int32_t qps_set_shared_polish(qps_handle h, int32_t on /* 1: every qps_solve_batch ends with the step; 0 (default): as without it */);

/* Adjoint derivatives of the solution on a shared-matrix batch handle (dense, sparse or CG): how a loss on x* changes with q, l, u and with the stored values of
 * P and A -- OSQP's adjoint_derivative_compute / _get_vec / _get_mat, for every column at once.  Per column, from a solution x, the multipliers y and
 * gx = dloss/dx: the active sets are those of the polishing step (L = {y_i < 0}, U = {y_i > 0}), K = [P, A_L', A_U'; A_L, 0, 0; A_U, 0, 0] is its reduced KKT
 * matrix, and K r = [gx; 0] is solved by its refinement rounds (MINRES on K + blkdiag(delta I, -delta I), all columns in lockstep on 16-column panels, every
 * column with its own state).  With r_lambda the multiplier block at full length m (zero outside the active sets):
 *     dq = -r_x,      dl_i = r_lambda_i on L, else 0,      du_i = r_lambda_i on U, else 0,
 *     dP_ij = -(r_x_i x_j + r_x_j x_i) / 2 for every stored entry of P (the gradient over symmetric perturbations: P is stored in full),
 *     dA_ij = -(y_i r_x_j + r_lambda_i x_j) for every stored entry of A (exactly 0 on a row outside the active sets),
 * dP and dA summed over the columns of the batch, since the columns share P and A.  dP_nzval and dA_nzval come in the order qps_get_shared_pattern hands out and
 * qps_update_shared_values takes; they are accumulated in double, also on a QPS_F32 handle, in a fixed order: two runs agree bit for bit.  The step reads
 * neither q, l nor u.  x and gx are [count][n]; y is [count][m], NULL takes the y the handle holds, as in qps_polish_shared.  The call uses numItrPolish, delta,
 * epsMinres and numItrMinres of *params and nothing else of it, and leaves everything the handle keeps untouched -- stored z and y, factor, options,
 * certificate: a following qps_solve_batch is bit for bit what it would have been.  A column whose last MINRES call ended with a flag other than 0 gets zeros in
 * its rows of dq, dl, du and is left out of the sums dP, dA; reports[b].flag says so, and the other report fields have the meaning of qps_polish_report.
 * Equilibration: the system is solved on the scaled data the handle holds, from D gx; r_x = D r~_x and r_lambda = E r~_lambda are exact powers of two, and
 * every output is in the caller's units.  The derivatives hold while the active sets do not change.
 * QPS_ERR_BAD_ARGUMENT: a NULL handle, x, gx or params, a NaN / Inf in x, y or gx, a delta that is not finite, a NaN epsMinres (before a device is needed; the
 * handle is unchanged).  QPS_ERR_UNSUPPORTED (qps_last_error names the reason): any handle that is not a shared-matrix batch; a non-NULL dP_nzval or dA_nzval
 * on a dense shared-matrix batch (dense matrix gradients are a panel GEMM: out of scope).
 * Out of scope: results in device memory, stand-alone handles, qps_create_dense_batch, ProxQP handles, derivatives across a change of the active set. */
int32_t qps_adjoint_shared(qps_handle h, const double *x, const double *y, const double *gx, const qps_params *params,
                           double *dq, double *dl, double *du,    /* [count][n], [count][m], [count][m]; any may be NULL */
                           double *dP_nzval, double *dA_nzval,    /* nnz(P), nnz(A) in the order of qps_get_shared_pattern; any may be NULL */
                           qps_polish_report *reports);           /* [count] or NULL */

/* Sparse shared-matrix batch: the same family of QPs on ONE sparse P (n x n, CSC, full symmetric storage) and ONE sparse A (m x n, CSC), index base 0 or 1
 * as for qps_create_csc -- a lasso / SVM regularisation path, a scenario sweep on a sparse model.  The linear system is the sparse L D L' of the KKT matrix
 * (QPS_LINSYS_KKT_LDL): ordering and symbolic factor are computed once, at creation, on the host (the QPS_LDL_* limits are read there, as a CSC handle reads
 * them at its first direct solve), one numeric factorisation serves every column, and every iteration sweeps 16 columns per launch.
 * Matrices are validated as by qps_create_csc, the vectors as by qps_create_dense_shared_batch for every column, before a device is needed; count <= 65535.
 * QPS_ERR_UNSUPPORTED from the create call: m = 0, or a pattern the level-scheduled plugin refuses (the analysis' message; still before a device is needed).
 * The handle is a batch handle like the dense one: qps_solve_batch, qps_get_dual, qps_update_shared_vectors, qps_set_profiling, qps_kernel_times,
 * qps_last_error and qps_destroy work on it, and column b behaves as a stand-alone qps_solve on a CSC handle with QPS_LINSYS_KKT_LDL and a fixed rho: its own
 * check, flag, iteration count and residuals; x, z, y are the iterates of its own stopping iteration.  A column of a batch equals the same data in a batch of
 * one bit for bit.
 * qps_solve_batch refuses with QPS_ERR_UNSUPPORTED (the handle stays usable): adptRho != 0, polish != 0, a linsys other than QPS_LINSYS_AUTO or
 * QPS_LINSYS_KKT_LDL (qps_params.polish stays refused; qps_polish_shared / qps_set_shared_polish run the step).  trsvBlock and loopVariant are accepted and without effect (they steer dense sweeps).  With reuseFactor = 1 and unchanged (rho, sigma)
 * nothing is factorised again, also after qps_update_shared_vectors.  qps_info per column: sweepVariant = 0, trsvBlock = 0, numRefactor = 0.
 * Environment, read once per handle at creation: QPS_LDL_PANEL_SPR = 1 | 4 | 16 forces that many 16-lane strips per factor row in every level of the sweeps
 * (unset: chosen per level from the mean row length). */
int32_t qps_create_csc_shared_batch(int64_t count, int64_t n, int64_t m, const int64_t *P_colptr, const int64_t *P_rowval, const double *P_nzval,
                                    const int64_t *A_colptr, const int64_t *A_rowval, const double *A_nzval, const double *q, const double *l,
                                    const double *u, int32_t index_base, int32_t dtype, int32_t device, qps_handle *out);

/* Matrix-free CG shared-matrix batch: the same family on ONE sparse P and ONE sparse A (CSC as above) with the matrix-free CG plugin (QPS_LINSYS_CG,
 * LinearSystemSolvers.jl:145-186) as its linear system -- for patterns that fill in under any ordering, which the L D L' handle refuses or cannot afford.
 * Nothing is analysed or factorised: every ADMM iteration runs one cg! per column, all columns in lockstep on 16-column panels, so the indices and values of
 * P, A and A' are read once per CG iteration for 16 columns and the four launches of a CG iteration are paid once per batch.  Every column has its own CG scalars
 * (tolerance max(sqrt(eps) ||r0||, epsPcg), at most numItrPcg iterations, x~ warm-started from the previous ADMM iteration and zero at the start of a solve) and
 * is a no-op from its last CG iteration on.
 * Arguments are validated as by qps_create_csc_shared_batch, in the same order, before a device is needed; instead of the n + m limit of the KKT matrix:
 * QPS_ERR_BAD_DIMENSION for n or m above 2^31 - 64.  QPS_ERR_UNSUPPORTED from the create call: m = 0.
 * The handle is a shared-matrix batch handle: qps_solve_batch, qps_get_dual, qps_update_shared_vectors, every qps_set_shared_* option but the equilibration,
 * qps_polish_shared, qps_set_profiling, qps_kernel_times, qps_last_error and qps_destroy work on it, and column b behaves as a stand-alone qps_solve on a CSC
 * handle with QPS_LINSYS_CG, matrix-free, at a fixed rho, with epsPcg and numItrPcg of qps_params: its own check, flag, iteration count and residuals.  Inner
 * products are added in an order that depends on n and the matrices only: a column of a batch equals the same data in a batch of one bit for bit.
 * A family-wide rho switch (qps_set_shared_adaptive_rho) and a per-row rho scale cost no factorisation here; numRefactor, rhoFinal and rhoProposed report the
 * switches as on the other handles.  qps_info.cgIterations of column b: the CG iterations of that column summed over the ADMM iterations of the solve.
 * qps_solve_batch refuses with QPS_ERR_UNSUPPORTED (the handle stays usable): adptRho != 0, polish != 0, a linsys other than QPS_LINSYS_AUTO or QPS_LINSYS_CG;
 * with QPS_ERR_BAD_ARGUMENT: an epsPcg that is negative or not finite, numItrPcg < 1.  reuseFactor, trsvBlock and loopVariant are accepted and without effect.
 * qps_set_shared_equilibration with passes > 0: QPS_ERR_UNSUPPORTED (passes = 0 is a no-op; qps_get_shared_equilibration returns ones). */
int32_t qps_create_csc_shared_batch_cg(int64_t count, int64_t n, int64_t m, const int64_t *P_colptr, const int64_t *P_rowval, const double *P_nzval,
                                       const int64_t *A_colptr, const int64_t *A_rowval, const double *A_nzval, const double *q, const double *l,
                                       const double *u, int32_t index_base, int32_t dtype, int32_t device, qps_handle *out);

/* New values of P and / or A on a shared-matrix batch handle, in place (OSQP's update_P_A): a linear time-varying MPC, an SQP outer loop or a re-linearised
 * scenario model keeps the shape and the sparsity pattern and changes the values at every sample.  qps_update_shared_matrices serves the dense handle (P n x n,
 * ldp; A m x n, lda; column-major as at creation), qps_update_shared_matrices_csc the sparse L D L' and the CG handle (CSC, index base 0 or 1); n, m and count
 * are the handle's.  A NULL matrix is kept -- for the CSC form the three pointers of a matrix are all NULL or all given -- and with both NULL the call returns
 * QPS_OK and changes nothing: the factor stays valid.  A given matrix is validated by the code of the creators (leading dimension, NaN / Inf,
 * issymmetric(mP) with tolerance 0, the CSC field checks), with their codes and messages, before a device is needed.  The arrays are copied.
 * Pattern (CSC form): the arrays are made canonical as at creation (rows sorted, duplicates summed) and colptr and rowval must then equal the handle's exactly; an
 * explicit zero is part of the pattern.  Anything else: QPS_ERR_BAD_ARGUMENT, qps_last_error names the matrix and the first column that differs.
 * Kept: every qps_set_shared_* option with its device buffers, q, l, u, the stored z and y (qps_set_shared_warm_start continues from them across the change),
 * the ordering, the symbolic factor, every index array and every allocation.  The sparse handles build, at their first update and not before, the position of every
 * entry of their by-rows copy of A in CSC order (and, while equilibrated, one exponent per stored entry); an update is then one upload of the values as doubles
 * and one launch per value array.
 * Stale afterwards: the numeric factor -- the next qps_solve_batch factorises even with reuseFactor = 1, as after qps_set_shared_rho_scale (sparse: the numeric
 * L D L' on the frozen pattern; CG: nothing to factorise); the dense handle's cached A'A only when A was given (with reuseFactor = 1 a P-only update
 * re-assembles and runs the Cholesky without the symmetric product), its diag(sqrt(scale)) A is re-formed when a rho scale is set and A was given; and
 * qps_get_shared_certificate returns zeros until the next solve.
 * Equilibration on: the exponents are kept, as in OSQP -- the handle stores D P D and E A D with the D, E it has, qps_get_shared_equilibration returns the same
 * vectors before and after, and a scaling computed from the new matrices is one more qps_set_shared_equilibration(h, passes).  The range check of that call runs on
 * the new values under the kept exponents before anything is modified (QPS_ERR_UNSUPPORTED).
 * After any refused call the handle is bit for bit what it was: matrices, factor validity, options and state.  The call returns with the handle's stream idle.
 * QPS_ERR_BAD_ARGUMENT: a NULL handle.  QPS_ERR_UNSUPPORTED (qps_last_error names the reason): the dense entry point on a sparse or CG handle, the CSC entry
 * point on a dense handle, either on a handle that is not a shared-matrix batch.
 * Out of scope: a change of pattern or shape, a scaling recomputed inside the update, stand-alone handles, qps_create_dense_batch and ProxQP handles. */
int32_t qps_update_shared_matrices(qps_handle h, const double *P, int64_t ldp, const double *A, int64_t lda);
int32_t qps_update_shared_matrices_csc(qps_handle h, const int64_t *P_colptr, const int64_t *P_rowval, const double *P_nzval, const int64_t *A_colptr,
                                       const int64_t *A_rowval, const double *A_nzval, int32_t index_base);

/* Values-only update of the sparse L D L' and the CG shared-matrix batch handle.  qps_update_shared_matrices_csc re-proves on the host, at every call, a pattern
 * that is frozen by contract (conversion, field checks, transposition of P, canonical form, pattern comparison); these two entry points skip all of it: the caller
 * reads the handle's canonical pattern once and from then on sends values only, in that order.  What still has to hold for VALUES is tested on the device.
 * qps_get_shared_pattern: the canonical pattern the handle was created on -- 0-based, rows sorted inside every column, duplicates summed, explicit zeros kept.
 * P_colptr and A_colptr have n + 1 elements, P_rowval *nnzP, A_rowval *nnzA; any output pointer may be NULL, so a first call sizes the arrays.  The pattern never
 * changes.  QPS_ERR_BAD_ARGUMENT: a NULL handle; QPS_ERR_UNSUPPORTED: a dense shared-matrix batch (it stores no pattern), a handle that is not a shared-matrix
 * batch.
 * qps_update_shared_values: P_nzval[nnzP] and / or A_nzval[nnzA], entry k the value of entry k of that pattern.  A NULL matrix is kept and its count ignored; both
 * NULL: QPS_OK, nothing changes, the factor stays valid.  location = QPS_MEM_HOST: host arrays, copied before the call returns.  location = QPS_MEM_DEVICE: the
 * pointers are device memory on the handle's device (hipMalloc or an allocator on top of it); CONTRACT: the work that produced the values has completed before the
 * call -- the handle copies them device to device on its own non-blocking stream, which is ordered against no stream of the caller (synchronise the producing
 * stream, or wait for an event recorded on it, first).  The arrays are free again when the call returns.
 * Tests, in the order of qps_update_shared_matrices_csc and with its codes and texts, so the same values are refused alike by both entry points: a count that
 * is not the handle's (QPS_ERR_BAD_ARGUMENT, naming the matrix and both counts), a location other than 0 / 1 (QPS_ERR_BAD_ARGUMENT), with QPS_MEM_DEVICE a pointer
 * that hipPointerGetAttributes does not call device memory of the handle's device (QPS_ERR_BAD_ARGUMENT, decided on the host before anything is enqueued); then, on
 * the device, on the staged doubles and before any value array of the handle is touched: NaN / Inf in P, then in A (QPS_ERR_NOT_FINITE, "P contains NaN/Inf"),
 * issymmetric(mP) with tolerance 0 -- entry (i, j) equals the stored entry (j, i), or equals 0 where (j, i) is not stored; the message names the column the host
 * test names -- (QPS_ERR_BAD_ARGUMENT), and, on the L D L' handle while equilibrated, the range of the entries under the kept exponents (QPS_ERR_UNSUPPORTED).
 * The host reads one verdict block (one copy, one synchronisation) and only then launches the value refresh of qps_update_shared_matrices_csc.
 * Kept, stale, equilibration: exactly as qps_update_shared_matrices_csc -- every option, q, l, u, z, y, the analysis and the exponents stay; the numeric factor goes
 * stale; certificates read zero until the next solve.  An updated handle equals, bit for bit, the handle that took the same values through
 * qps_update_shared_matrices_csc.  The handle builds at its first call, and keeps, the position of every entry's transpose partner in P (nnzP ints).  The L D L'
 * handle keeps its host copy of the values current (device input: one device-to-host copy of the committed doubles inside the call), so a later
 * qps_set_shared_equilibration computes its exponents from the new matrices; the CG handle keeps no host values.
 * After any refused call the handle is bit for bit what it was (the staging may hold the refused values).  The call returns with the handle's stream idle.
 * QPS_ERR_UNSUPPORTED: a dense shared-matrix batch (use qps_update_shared_matrices), a handle that is not a shared-matrix batch.
 * Out of scope: a mode without validation, a change of pattern, q / l / u or results in device memory, capturing the call in a graph. */
#define QPS_MEM_HOST   0
#define QPS_MEM_DEVICE 1
int32_t qps_get_shared_pattern(qps_handle h, int64_t *nnzP, int64_t *nnzA, int64_t *P_colptr, int64_t *P_rowval, int64_t *A_colptr, int64_t *A_rowval);
int32_t qps_update_shared_values(qps_handle h, const double *P_nzval, int64_t nnzP, const double *A_nzval, int64_t nnzA, int32_t location);

/* The per-problem loop of RunBenchmarks.jl:88-104 sharded over the devices of ONE process ("one host thread + one stream per device", "work-stealing at
 * chunk boundaries").  `count` independent dense QPs of one shape, arrays stacked as for qps_create_dense_batch; `devices[num_workers]` lists the device of every worker
 * -- one host thread each; a device may be listed more than once (two workers sharing a card).  Every worker repeatedly takes the next range of QPs from a shared
 * counter -- `chunk` of them at first, fewer towards the end of the batch: clamp(ceil(remaining / (2 W)), max(1, chunk / 4), chunk) -- builds a batch handle for them on
 * its device, solves them (qps_solve_batch) and drops the handle: a run to a tolerance, in which every QP stops at its own iteration, balances itself.  chunk <= 0:
 * static contiguous slabs, worker w takes QPs [w * ceil(count / W), ...) -- what a fixed-K run wants (equal work per QP, no hand-out).  The size of a range depends
 * only on where it starts, so the ranges are cut the same way whoever solves them: the results do not depend on timing or on which worker took a range, and they
 * equal qps_solve_batch on batches of those same ranges bit for bit.  No data-path collective, no exchange between devices.
 * x_inout [count][n] (warm starts in, solutions out), infos [count] (may be NULL), worker_of [count] (may be NULL: which worker solved QP b), worker_seconds
 * [num_workers] (may be NULL: busy time per worker, handle creation included).  On an error the other workers stop at their next chunk boundary and the first error is
 * returned (qps_last_error(NULL) on the calling thread). */
int32_t qps_solve_batch_multi(int64_t count, int64_t n, int64_t m, const double *P, const double *A, const double *q, const double *l, const double *u,
                              int32_t dtype, const int32_t *devices, int32_t num_workers, int32_t chunk, double *x_inout, const qps_params *p, qps_info *infos,
                              int32_t *worker_of, double *worker_seconds);

/* Device-time of the loop kernels of the last qps_solve, measured with HIP events attached to the kernel dispatches
 * themselves (hipExtLaunchKernelGGL start / stop events on the solver's stream: the dispatch's own begin / end timestamps)
 * (used by bench.py's roofline block).  names is a caller buffer of `cap` entries; returns the number filled. */
typedef struct { char name[48]; double seconds; int64_t launches; double algo_bytes; } qps_kernel_time;
int32_t qps_kernel_times(qps_handle h, qps_kernel_time *out, int32_t cap, int32_t *count);
/* level 0 = off; 1 = sampling: once per 50 iterations ONE launch of each loop kernel (fused pass, fused sweeps, the two slab
 * reductions; each on a different iteration) is bracketed with HIP events -- cheap enough for a timed region (an event pair
 * per launch would cost ~7 % of the loop);
 * 2 = bracket every loop kernel (diagnostic).  Setting the level also resets the accumulated times. */
int32_t qps_set_profiling(qps_handle h, int32_t on);

/* ---- The reference's second solver form (ProxQP.jl):  min 1/2 x'Px + q'x  s.t.  A x = b,  C x <= d ---------------------------
 * qps_proxqp_create_dense  == the data half of  ProxQP(mP, vQ, mA, vB, mC, vD [, vX, vY, vZ, vS])        ProxQP.jl:36,73
 * qps_proxqp_init_kkt      == the initialisation of the 6-argument constructor (x, y from the equality-constrained KKT
 *                             system, s = max(d - C x, 0), z = 0)                                        ProxQP.jl:80-89
 * qps_proxqp_set_state     == the explicit vX, vY, vZ, vS of the 10-argument constructor                 ProxQP.jl:36
 * qps_proxqp_solve         == SolveQuadraticProgram!(sQpProb; numIterations, ϵAbs, ϵRel, numItrConv, ρ, σ, adptΡ, τ) -> dReport
 *                             (always runs numIterations: the reference's `break` is commented out)      ProxQP.jl:118-173
 * qps_proxqp_get_state     == reading sQpProb.vX / vY / vZ / vS afterwards
 * All matrices column-major (Julia Matrix{Float64}); numEq or numInEq may be 0.  Same handle type, qps_destroy frees it. */
typedef struct {
    int32_t numIterations;   /* 2000 */
    int32_t numItrConv;      /* 50 */
    int32_t adptRho;         /* adptΡ, default 1 */
    int32_t loopVariant;     /* additive: 0 = auto (one fused pass over [A; C] per iteration), 1 = unfused (two passes) */
    double epsAbs;           /* ϵAbs 1e-7 */
    double epsRel;           /* ϵRel 1e-6 */
    double rho;              /* ρ 1e2 */
    double sigma;            /* σ 1e-2 */
    double tau;              /* τ 10 */
} qps_proxqp_params;
typedef struct {             /* dReport (ProxQP.jl:127): "Converged", "Iterations", "ρ", "σ", "PrimalResidual", "DualResidual" */
    int32_t converged; int32_t iterations; double rho, sigma, resPrim, resDual;
} qps_proxqp_report;
int32_t qps_proxqp_default_params(qps_proxqp_params *p);
int32_t qps_proxqp_create_dense(int64_t n, int64_t numEq, int64_t numInEq, const double *P, int64_t ldp, const double *q,
                                const double *A, int64_t lda, const double *b, const double *C, int64_t ldc, const double *d,
                                int32_t dtype, int32_t device, qps_handle *out);
/* SparseProxQP (ProxQP.jl:71, :95-115): the same with the colptr / rowval / nzval fields of three SparseMatrixCSC inputs (index_base 1 for
 * Julia).  The matrices stay sparse: the linear system of UpdateX! (:221-225) is solved in its KKT form [P + sigma I, G'; G, -I/rho], G = [A; C],
 * by the sparse L D L' plugin -- ordering and symbolic factor once per handle, a rho update re-factorises numerically on the frozen pattern
 * (the role of AlignSparsePattern / GetNzvalDiagIdxs / UpdateM! / the pattern-reusing cholesky!, :184-190, :201-206, :335-372).
 * qps_proxqp_init_kkt on such a handle: sparse factor of [P A'; A -1e-8 I] + iterative refinement against [P A'; A 0] (:95-115).
 * QPS_ERR_UNSUPPORTED at the first solve / init when the factor does not fit the level-scheduled plugin (then: the dense constructor). */
int32_t qps_proxqp_create_csc(int64_t n, int64_t numEq, int64_t numInEq, const int64_t *P_colptr, const int64_t *P_rowval, const double *P_nzval,
                              const double *q, const int64_t *A_colptr, const int64_t *A_rowval, const double *A_nzval, const double *b,
                              const int64_t *C_colptr, const int64_t *C_rowval, const double *C_nzval, const double *d, int32_t index_base,
                              int32_t dtype, int32_t device, qps_handle *out);
int32_t qps_proxqp_init_kkt(qps_handle h);
int32_t qps_proxqp_set_state(qps_handle h, const double *x, const double *y, const double *z, const double *s);
int32_t qps_proxqp_get_state(qps_handle h, double *x, double *y, double *z, double *s);
int32_t qps_proxqp_solve(qps_handle h, const qps_proxqp_params *params, qps_proxqp_report *report);

/* The modeAuto rule of SolveQuadraticProgramRef! (SolveQuadraticProgram.jl:129-130, :143-151; SolveQuadraticProgram.m:190-199):
 * numRowsL = n + m, nnzDensity = (nnz(P) + nnz(A)) / numRowsL^2; direct when numRowsL <= 5000 and nnzDensity <= 0.4, else
 * iterative.  Returns the qps_linsys_kind to use: QPS_LINSYS_CG (iterative), or for "direct" QPS_LINSYS_KKT_LDL when the caller
 * holds sparse matrices (sparse_input != 0; the reference's ldlt / decomposition(...,'ldl') of the sparse KKT matrix) and
 * QPS_LINSYS_CHOLESKY for dense arrays.  Pure function: no handle, no device. */
int32_t qps_linsys_auto(int64_t n, int64_t m, int64_t nnzP, int64_t nnzA, int32_t sparse_input);

/* Symbolic analysis of the KKT matrix for QPS_LINSYS_KKT_LDL on its own (host only, no device needed): what LaLdlInit / QDLdlInit /
 * FacLdlInit do before the numeric factorisation (LinearSystemSolvers.jl:18, :49, :81).  perm_out (n + m entries, may be NULL)
 * receives the elimination order over [x; nu] in the caller's index base; the report sizes the factor. */
typedef struct {
    int64_t numRows;            /* n + m */
    int64_t numSparseColumns;   /* columns kept as scalar sparse columns (wide elimination-tree levels) */
    int64_t tailSize;           /* columns near the root handled as one dense block */
    int64_t numSparseLevels;    /* launches per triangular sweep over the sparse part */
    int64_t treeHeight;         /* height of the elimination tree */
    int64_t nnzK;               /* strictly lower triangle of K */
    int64_t nnzL;               /* strictly lower triangle of L under the minimum-degree ordering */
    int64_t nnzStored;          /* entries actually stored (the tail counted as dense) */
} qps_ldl_report;
int32_t qps_ldl_analyze(int64_t n, int64_t m, const int64_t *P_colptr, const int64_t *P_rowval, const int64_t *A_colptr,
                        const int64_t *A_rowval, int32_t index_base, int64_t *perm_out, qps_ldl_report *report);

int32_t qps_destroy(qps_handle h);
/* Human-readable description of the last failure on this handle (or of the last failed create when h == NULL). */
const char *qps_last_error(qps_handle h);
const char *qps_version(void);

#ifdef __cplusplus
}
#endif
#endif /* QPS_H */
