/*
 * permon_hip.h -- C ABI of libpermonhip: an MI355X (gfx950) implementation of PERMON's QPS hot path.
 *
 * Drop-in boundary.  PERMON reaches its numerical kernels through three op tables and a handful of
 * Mat implementations; every entry point below names the reference slot it replaces
 * (file:line under /root/reference).  INTEGRATION.md shows the PETSc-side glue that binds them.
 *
 *   - all vector arguments are DEVICE pointers to fp64 (PetscScalar = double, real build);
 *     index arrays handed to *_create functions are HOST pointers (copied to the device once);
 *   - every function returns 0 (PETSC_SUCCESS) or a non-zero pmh error code; pmh_last_error()
 *     returns the message.  Solver failure is NOT an error: it is reason < 0 (qps.c:551);
 *   - no function falls back to a CPU path: without a usable HIP device pmh_init() fails.
 *   - one pmh context per process = one GPU (one MPI rank <-> one GPU, matblockdiag.c:787-788).
 */
#ifndef PERMON_HIP_H
#define PERMON_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- errors ------------------------------------------------------------------------------------ */
#define PMH_SUCCESS 0
#define PMH_ERR_HIP 1       /* HIP runtime error (message has the hipError string) */
#define PMH_ERR_ARG 2       /* bad argument (PETSC_ERR_ARG_*) */
#define PMH_ERR_STATE 3     /* wrong state (PETSC_ERR_ARG_WRONGSTATE / PETSC_ERR_ORDER) */
#define PMH_ERR_SUP 4       /* unsupported (PETSC_ERR_SUP) */
#define PMH_ERR_NODEVICE 5  /* no gfx950 device / extension unusable */
#define PMH_ERR_COMM 6      /* RCCL error */
const char *pmh_last_error(void);

/* KSPConvergedReason values the path produces (PETSc petscksp.h; qps.c:675-714, smalxe.c:610-692) */
#define PMH_CONVERGED_ITERATING 0
#define PMH_CONVERGED_RTOL 2
#define PMH_CONVERGED_ATOL 3
#define PMH_CONVERGED_ITS 4
#define PMH_CONVERGED_HAPPY_BREAKDOWN 7
#define PMH_DIVERGED_ITS (-3)
#define PMH_DIVERGED_DTOL (-4)
#define PMH_DIVERGED_BREAKDOWN (-5)
#define PMH_DIVERGED_NANORINF (-9)
#define PMH_DECIDE (-1.0) /* PETSC_DECIDE */

/* ---- context, memory, multi-GPU communicator ----------------------------------------------------- */
typedef struct pmh_ctx_s *pmh_ctx;

int pmh_init(int device, pmh_ctx *ctx);     /* PermonInitialize's device part; fails loudly without a GPU */
/* Process-wide run-time switches (the role of PETSc's options database for the library's own A/B switches; the environment variable PMH_<NAME> gives the initial value).
 * "chain" (PMH_NO_CHAIN unset = 1): the penalised, projected FETI operator as the five-launch dual-space chain (dualchain.hip); 0 = the round-4 launch sequence.
 * Takes effect for operators created afterwards.  "chain_applies" / "chain_launches": counters of the chain's applications and of its own kernel launches (the middle
 * stage's -- GEMM + finishing launch, or the inner Krylov solve -- not included); set to reset.  "chain_replay" (PMH_NO_CHAIN_REPLAY unset = 1): where SMALXE and its
 * inner MPGP multiply the same iterate twice in a row (objective, first gradient of the next inner solve) the chain runs only its last kernel on the intermediates it
 * kept -- the same bits, no product with F; 0 = every application is the full chain.  "chain_replays": counter of such applications (each also counts in "chain_applies");
 * "chain_replays_redone": how many of them were taken again in full because the inner solve's projection onto the box had changed the iterate; set to reset.  "host_threads": threads of the host-side set-up builders (3x3-block
 * copies, multigrid hierarchy, class detection); initial value PMH_HOST_THREADS, else OMP_NUM_THREADS, else min(16, the CPUs the process may run on) -- with several ranks
 * per node every rank must get its share.  "svm_pairing" (PMH_SVM_NO_PAIRING unset = 1): the SVM dual's paired passes over X inside MPGP; 0 = every Hessian application as its
 * own two passes (may change between two solves; every rank of a job must set it alike).  "gt_fusion" (PMH_NO_GT_FUSION), "smalxe_prefetch" (PMH_SMALXE_NO_PREFETCH),
 * "mg_d0_fusion" (PMH_MG_NO_D0_FUSION): A/B switches of fusions on per-product paths, 1 = fused (the default).  "orbit_adapted" (PMH_NO_ORBIT_ADAPTED unset = 1): a class of
 * PMH_FX_CLASS_ORBIT with all 48 operations of the cube (pmh_fexplicit_set_box_symmetry) on one rank applies W_c in the group's symmetry-adapted basis (fshared_adapted.h)
 * instead of the orbit GEMM; read at the assembly and at every application, 0 = the GEMM.  "orbit_adapted_classes": counter of classes that took that form at their assembly,
 * "orbit_adapted_fallbacks": of classes that were eligible but failed the set-up's self-check against the GEMM and stayed on it; set to reset.  "orbit_adapted_spoil" (tests):
 * 1 = the next assembly builds its basis with one table row negated, which the self-check must catch.  "orbit_narrow" (tests' A/B, default 1): read at the assembly; a class on
 * that form whose multivector has at most 16 columns (two groups of 8 blocks) runs the transforms sized for it (k_fxa_narrow), 0 = the wide transforms for every width; the
 * results are the same bits either way.  Unknown name: PMH_ERR_ARG. */
int pmh_set_knob(const char *name, int value);
int pmh_get_knob(const char *name, int *value);
int pmh_finalize(pmh_ctx ctx);
int pmh_mem_info(pmh_ctx ctx, size_t *free_bytes, size_t *total_bytes); /* HBM of the context's device */
int pmh_device_name(pmh_ctx ctx, char *buf, size_t len);
int pmh_sync(pmh_ctx ctx);                  /* hipStreamSynchronize of the context's compute stream */
void *pmh_stream(pmh_ctx ctx);              /* the hipStream_t kernels are launched on */

int pmh_malloc(pmh_ctx ctx, size_t bytes, void **dptr);
int pmh_free(pmh_ctx ctx, void *dptr);
int pmh_memcpy_h2d(pmh_ctx ctx, void *dst, const void *src, size_t bytes);
int pmh_memcpy_d2h(pmh_ctx ctx, void *dst, const void *src, size_t bytes);
int pmh_memcpy_d2d(pmh_ctx ctx, void *dst, const void *src, size_t bytes);
int pmh_memset(pmh_ctx ctx, void *dst, int value, size_t bytes);

/* timing on the compute stream with HIP events (bench.py's roofline leg) */
int pmh_timer_start(pmh_ctx ctx);
int pmh_timer_stop(pmh_ctx ctx, double *milliseconds);

/* RCCL communicator over xGMI: replaces the MPI_Allreduce / PetscSF / VecScatter call sites of SURVEY 2.4 */
#define PMH_UNIQUE_ID_BYTES 128
int pmh_comm_unique_id(void *id128);                                     /* rank 0, then broadcast out of band */
int pmh_comm_init(pmh_ctx ctx, int rank, int size, const void *id128);  /* collective */
int pmh_comm_rank(pmh_ctx ctx, int *rank, int *size);
int pmh_comm_allreduce_sum(pmh_ctx ctx, double *dbuf, size_t count);    /* in place, device buffer */
int pmh_comm_allreduce_min(pmh_ctx ctx, double *dbuf, size_t count);
int pmh_comm_barrier(pmh_ctx ctx);
/* HIP-event pairs (on the launch stream) around the next max_events vector all-reduces of the data path -- the sum of the ranks' B u that ends MatMultTranspose_Gluing
 * (PetscSFReduce, gluing.c:144-147); 0 switches the timing off.  _get: how many were timed, their total milliseconds and bytes; resets the counters. */
int pmh_comm_timing_enable(pmh_ctx ctx, int max_events);
int pmh_comm_timing_get(pmh_ctx ctx, int *count, double *total_ms, double *bytes);
/* Host-staged transport instead of RCCL: every collective of the data path (B u in pmh_gluing_mult_transpose, the SVM w, the grouped MPGP scalars, the barrier) copies its
 * device buffer to pinned host memory and calls fn -- an IN-PLACE all-reduce over the ranks (op: PMH_COMM_SUM / PMH_COMM_MIN; PMH_COMM_BARRIER with count 0), returning 0 on
 * success -- then copies the result back, in stream order.  What the PETSc glue passes when the ranks cannot form an RCCL communicator: MPI_Allreduce(MPI_IN_PLACE, buf, count,
 * MPI_DOUBLE, MPI_SUM / MPI_MIN, comm) (replaces the reference's MPI reductions: gluing.c:144-147, qpc.c:521, VecDot / VecNorm).  fn == NULL removes it.  Not together with pmh_comm_init. */
enum { PMH_COMM_SUM = 0, PMH_COMM_MIN = 1, PMH_COMM_BARRIER = 2 };
typedef int (*pmh_comm_host_fn)(void *user, int op, double *host_buf, size_t count);
int pmh_comm_set_host_transport(pmh_ctx ctx, int rank, int size, pmh_comm_host_fn fn, void *user);

/* ---- Mat: CSR (PETSc SeqAIJ role) ---------------------------------------------------------------- */
/* replaces MatMult(A,..) at mpgp.c:500,537,578,606,624, mpgp.c:250, permonmatutils.c:487,
   matblockdiag.c:197 (local block), extension.c:485,519 (condensed block) */
typedef struct pmh_csr_s *pmh_csr;
int pmh_csr_create(pmh_ctx ctx, int nrows, int ncols, const int *rowptr, const int *col, const double *val, pmh_csr *A);
int pmh_csr_destroy(pmh_csr A);
int pmh_csr_sizes(pmh_csr A, int *nrows, int *ncols, long long *nnz);
int pmh_csr_mult(pmh_csr A, const double *x, double *y);                       /* y = A x       */
int pmh_csr_mult_add(pmh_csr A, const double *x, const double *y1, double *y);  /* y = y1 + A x  */
int pmh_csr_mult_transpose(pmh_csr A, const double *x, double *y);             /* y = A' x      */
int pmh_csr_mult_transpose_add(pmh_csr A, const double *x, const double *y1, double *y); /* y = y1 + A' x */
int pmh_csr_algorithmic_bytes(pmh_csr A, double *bytes);                        /* 12 nnz + 20 nrows */
/* per-launch kernel timing with HIP events on the launch stream (bench.py's roofline leg): every SpMV launch of A
   is bracketed by an event pair while enabled; `epilogue` selects 0 plain, 1 mult-add, 2 fused "-b", 3 fused MPGP phase P1 */
int pmh_csr_timing_enable(pmh_csr A, int max_launches);
int pmh_csr_timing_get(pmh_csr A, int epilogue, int *launches, double *total_ms);

/* ---- generic operator (PETSc Mat with a mult slot) ------------------------------------------------ */
typedef struct pmh_op_s *pmh_op;
typedef int (*pmh_shell_mult_fn)(void *user, const double *x_dev, double *y_dev);
int pmh_op_create_csr(pmh_csr A, pmh_op *op);                           /* borrows A */
int pmh_op_create_shell(pmh_ctx ctx, int n, pmh_shell_mult_fn f, void *user, pmh_op *op); /* MatCreateShellPermon, shell.c:5-31 */
int pmh_op_destroy(pmh_op op);
int pmh_op_size(pmh_op op, int *n);
int pmh_op_mult(pmh_op op, const double *x, double *y);
int pmh_op_mult_transpose(pmh_op op, const double *x, double *y); /* MatMultTranspose; PMH_ERR_SUP for a shell without the slot */
/* MatGetMaxEigenvalue, src/mat/interface/permonmatutils.c:442-522 (tol/maxits: PMH_DECIDE -> 1e-4 / 50) */
int pmh_op_max_eigenvalue(pmh_op op, double tol, int maxits, double *lambda, int *its);

/* ---- QPC box: struct _QPCOps slots (include/permon/private/qpcimpl.h:8-25) ------------------------- */
/* lb / ub may be NULL (no bound of that kind).  n = local length of the constrained (sub)vector. */
int pmh_qpc_box_project(pmh_ctx ctx, int n, const double *x, const double *lb, const double *ub, double *Px);     /* QPCProject_Box qpcbox.c:290-305 */
int pmh_qpc_box_feas(pmh_ctx ctx, int n, const double *x, const double *d, const double *lb, const double *ub, double *alpha_host); /* QPCFeas_Box qpcbox.c:104-146; the MIN all-reduce of qpc.c:521 has no counterpart: constrained vectors are replicated */
int pmh_qpc_box_grads(pmh_ctx ctx, int n, const double *x, const double *g, const double *lb, const double *ub, double astol, double *gf, double *gc); /* QPCGrads qpc.c:540-569 + QPCGrads_Box qpcbox.c:21-64 */
int pmh_qpc_box_gradreduced(pmh_ctx ctx, int n, const double *x, const double *gf, const double *lb, const double *ub, double alpha, double *gr); /* QPCGradReduced qpc.c:589-615 + _Box qpcbox.c:68-100 */
/* expands an index-set restricted bound (qpc->is, qpc.c:416-437) to a full-length bound with -inf/+inf elsewhere */
int pmh_qpc_box_expand_is(pmh_ctx ctx, int n, int nis, const int *is_host, const double *bound_sub, double fill, double *bound_full);

/* ---- post-solve: KKT residuals of a box-constrained QP -------------------------------------------------------- */
/* QPComputeMissingBoxMultipliers (qp.c:828-893: lambda_lb = A x - b, lambda_ub = -(A x - b), both clipped at 0 when both
   bounds exist) + the `r = ...` lines of QPViewKKT (qp.c:245-369) and QPCViewKKT_Box (qpcbox.c:333-427).
   out[0] = ||A x - b - lambda_lb + lambda_ub||, out[1] = ||min(x-lb,0)||, out[2] = ||min(lambda_lb,0)||,
   out[3] = |lambda_lb'(lb-x)|, out[4] = ||max(x-ub,0)||, out[5] = ||min(lambda_ub,0)||, out[6] = |lambda_ub'(x-ub)|,
   out[7] = ||b||  (entries of an absent bound are 0).  work: device scratch of length n. */
int pmh_qp_kkt_box(pmh_op A, const double *b, const double *x, const double *lb, const double *ub, double *work, double out_host[8]);

/* ---- Vec kernels used by the path (PETSc VecAXPY/AYPX/WAXPY/Dot/Norm/Copy/Set/Scale) --------------- */
int pmh_vec_axpy(pmh_ctx ctx, int n, double *y, double a, const double *x);                  /* y += a x */
int pmh_vec_aypx(pmh_ctx ctx, int n, double *y, double a, const double *x);                  /* y = x + a y */
int pmh_vec_waxpy(pmh_ctx ctx, int n, double *w, double a, const double *x, const double *y); /* w = a x + y */
int pmh_vec_scale(pmh_ctx ctx, int n, double *x, double a);
int pmh_vec_set(pmh_ctx ctx, int n, double *x, double a);
int pmh_vec_copy(pmh_ctx ctx, int n, const double *x, double *y);
int pmh_vec_dot(pmh_ctx ctx, int n, const double *x, const double *y, double *result_host);
int pmh_vec_norm2(pmh_ctx ctx, int n, const double *x, double *result_host);

/* ---- QPS MPGP: struct _QPSOps.solve / .setup  (src/qps/impls/mpgp/mpgp.c:359-650) ------------------- */
enum { PMH_EXP_STD = 0, PMH_EXP_PROJCG, PMH_EXP_GF, PMH_EXP_G, PMH_EXP_GFGR, PMH_EXP_GGR };           /* QPSMPGPExpansionTypes, mpgp.c:3 */
enum { PMH_EXPLEN_FIXED = 0, PMH_EXPLEN_OPT, PMH_EXPLEN_OPTAPPROX, PMH_EXPLEN_BB };                    /* QPSMPGPExpansionLengthTypes, mpgp.c:4 */

typedef struct {
  /* QPS tolerances: QPSCreate qps.c:73-76 */
  double rtol, atol, divtol;
  int    max_it;
  /* QPS_MPGP: QPSCreate_MPGP mpgp.c:827-843 */
  double alpha_user;   /* PMH_DECIDE -> 2.0 */
  int    alpha_direct; /* QPS_ARG_DIRECT (1) / QPS_ARG_MULTIPLE (0) */
  double gamma;
  double maxeig;       /* PMH_DECIDE -> power method */
  double maxeig_tol;
  int    maxeig_iter;
  double bchop_tol;
  double astol;        /* qpc->astol, qpc.c:28: 10*eps */
  int    exptype, explengthtype;
  int    resetalpha, fallback, fallback2;
  int    monitor;      /* record the QPSMonitorDefault_MPGP trace (mpgp.c:21-34) */
  int    unfused;      /* 1: run the literal one-kernel-per-PETSc-call sequence (every variant supports it);
                          0: std expansion + fixed length without fallback takes the fused kernels */
  int    distributed;  /* 1: x, b, lb, ub are ROW-DISTRIBUTED over the ranks of the communicator (PETSc MPI Vec layout):
                          every dot / norm / min is completed with an RCCL all-reduce of the device scalars, replacing
                          VecDot's and QPCFeas' MPI_Allreduce.  0: vectors are rank-local or replicated */
} pmh_mpgp_opts;

typedef struct {
  int    iteration, reason;
  double rnorm, gfnorm, gcnorm, alpha, maxeig;
  int    nmv, ncg, nexp, nprop, nfinc, nfall;
  double norm_rhs, ttol;
  char   current_step_type;
} pmh_mpgp_stats;

typedef struct pmh_mpgp_s *pmh_mpgp;
int pmh_mpgp_default_opts(pmh_mpgp_opts *o);
/* QPSSetup_MPGP: work vectors, bound chop, power method, alpha. lb/ub full-length device vectors or NULL */
int pmh_mpgp_create(pmh_ctx ctx, pmh_op A, const double *b, double *x, const double *lb, const double *ub, const pmh_mpgp_opts *o, pmh_mpgp *s);
int pmh_mpgp_destroy(pmh_mpgp s);
int pmh_mpgp_solve(pmh_mpgp s);                                     /* QPSSolve_MPGP mpgp.c:438-650 */
int pmh_mpgp_get_stats(pmh_mpgp s, pmh_mpgp_stats *st);
/* qps->convergencetest (qps.c:675; called at mpgp.c:531 every iteration with rnorm / iteration current).
   The callback sets *reason (0 = keep iterating); NULL restores QPSConvergedDefault.  This is the hook
   SMALXE uses to inject QPSConverged_Inner_SMALXE (smalxe.c:874-875). */
typedef int (*pmh_converged_fn)(void *user, int iteration, double rnorm, int *reason);
int pmh_mpgp_set_convergence_test(pmh_mpgp s, pmh_converged_fn f, void *user);
int pmh_mpgp_set_tolerances(pmh_mpgp s, double rtol, double atol, double divtol, int max_it); /* QPSSetTolerances */
/* monitor trace: per iteration step type, ||gP||, ||gf||, ||gc||, alpha (arrays of length >= iteration+1) */
int pmh_mpgp_get_trace(pmh_mpgp s, int cap, char *step, double *gp, double *gf, double *gc, double *alpha, int *len);
int pmh_mpgp_get_work(pmh_mpgp s, int idx, const double **dptr);   /* work[0..6] = gP,gf,gc,g,p,Ap,gr (mpgp.c:6-17) */
/* composed methods SMALXE needs from its inner solver (mpgp.c:858-869) */
int pmh_mpgp_set_operator_max_eigenvalue(pmh_mpgp s, double maxeig);   /* "QPSMPGPSetOperatorMaxEigenvalue_MPGP_C" mpgp.c:107-115 */
int pmh_mpgp_update_max_eigenvalue(pmh_mpgp s, double maxeig_update);  /* "QPSMPGPUpdateMaxEigenvalue_MPGP_C"      mpgp.c:119-143 */
int pmh_mpgp_get_current_step_type(pmh_mpgp s, char *step);            /* "QPSMPGPGetCurrentStepType_MPGP_C"       mpgp.c:38-45  */
int pmh_mpgp_reset_statistics(pmh_mpgp s);                             /* QPSResetStatistics_MPGP mpgp.c:654-664 */
int pmh_mpgp_get_tolerances(pmh_mpgp s, double *rtol, double *atol, double *divtol, int *max_it); /* QPSGetTolerances; any pointer may be NULL */

/* ---- QPPF projector factory (src/qppf/interface/qppf.c) ----------------------------------------------- */
typedef struct pmh_qppf_s *pmh_qppf;
/* G: m x n CSR (device); GG' is formed and Cholesky-factored on the host once (QPPFSetUpGGt/GGtinv_Private
   qppf.c:213-333, MATINV monolithic direct solve), the factor is applied redundantly on the device.
   orthonormal == 1 <=> G_has_orthonormal_rows (GGtinv = NULL, qppf.c:225-229).
   orthonormal == 2: G is NOT orthonormal and is orthonormalised IMPLICITLY (QPTOrthonormalizeEq with -qp_E_orth_form implicit, the reference's default
   form, qptransform.c:647; MatOrthRows_Implicit_Default permonmatorth.c:176-205): the object behaves exactly as one created with the explicit
   T G (GG' = L L', T = L^{-1}; orthonormal rows) but keeps G as sparse as it came and applies the small dense T / T'T inside the finishing launch
   of G v.  The right-hand side of the constraint transforms with pmh_qppf_orth_rhs (e = T e0, host vectors of length m). */
int pmh_qppf_create(pmh_ctx ctx, pmh_csr G, int orthonormal, pmh_qppf *pf);
int pmh_qppf_orth_rhs(pmh_qppf pf, const double *e0_host, double *e_host);
/* One-row projector (the role of the reference's MATONEROW, src/mat/impls/onerow/onerow.c): G = a' for a dense device vector a of n doubles (borrowed), m = 1.
   No CSR and no host factorisation: G G' = a'a is one reduction at creation.  Every pmh_qppf_apply_* works on it (G v: one dot product; G's: one scaled copy;
   Q v = a (a'v) / (a'a)); the rows count as orthonormal where |a'a - 1| <= n eps.  Under a communicator a is sharded as the vectors are and the dot product is
   joined by pmh_comm_allreduce_sum.  pmh_op_create_penalized over the SVM dual operator and such a projector whose row is a multiple of the labels folds
   rho G'G into the operator (pmh_op_svm_dual_set_terms' rank-one term) instead of applying the projector */
int pmh_qppf_create_onerow(pmh_ctx ctx, const double *a_dev, int n, pmh_qppf *pf);
int pmh_qppf_destroy(pmh_qppf pf);
/* set-up cost of the coarse problem: GG' assembly on the matrix cores (ms, flops = 2 Mp^2 n) and the host Cholesky + inverse (ms) */
int pmh_qppf_setup_stats(pmh_qppf pf, double *ggt_mfma_ms, double *ggt_flops, double *host_inverse_ms);
int pmh_qppf_apply_Q(pmh_qppf pf, const double *v, double *Qv);     /* QPPFApplyQ   qppf.c:454-503 */
int pmh_qppf_apply_P(pmh_qppf pf, const double *v, double *Pv);     /* QPPFApplyP   qppf.c:563-575 */
int pmh_qppf_apply_GtG(pmh_qppf pf, const double *v, double *y);    /* QPPFApplyGtG qppf.c:580-605 */
int pmh_qppf_apply_CP(pmh_qppf pf, const double *x, double *y);     /* QPPFApplyCP  qppf.c:610-645: y = (GG')^{-1} x, length m */
int pmh_qppf_apply_halfQ(pmh_qppf pf, const double *x, double *y);  /* QPPFApplyHalfQ qppf.c:507-527 */
int pmh_qppf_apply_halfQ_transpose(pmh_qppf pf, const double *x, double *y); /* qppf.c:531-559 */
int pmh_qppf_apply_G(pmh_qppf pf, const double *v, double *Gv);     /* MatMult(cp->G,..) qppf.c:475 */

/* ---- composed operators of the QP transform chain ------------------------------------------------------ */
int pmh_op_create_penalized(pmh_op A, pmh_qppf pf, double rho, pmh_op *op);   /* MatCreatePenalized matpenalized.c:212-243; mult :12-22 */
/* the other three op slots MatCreatePenalized registers (matpenalized.c:232-235): MatMultTranspose_Penalized :26-36 (through
   pmh_op_mult_transpose), MatMultAdd_Penalized :40-57 (y = x2 + A_rho x; x2 may be y), MatMultTransposeAdd_Penalized :61-78 */
int pmh_op_penalized_mult_add(pmh_op op, const double *x, const double *x2, double *y);
int pmh_op_penalized_mult_transpose_add(pmh_op op, const double *x, const double *x2, double *y);
int pmh_op_penalized_set_penalty(pmh_op op, double rho);                      /* MatPenalizedSetPenalty */
int pmh_op_penalized_get_penalty(pmh_op op, double *rho);
int pmh_op_create_projected(pmh_op A, pmh_qppf pf, int symmetric, pmh_op *op); /* P*A*P (symmetric) or P*A: qptransform.c:273-284 */

/* ---- FETI Mats ------------------------------------------------------------------------------------------ */
/* MATGLUING (src/mat/impls/gluing/gluing.c): leaves (local primal dof, lambda index, sign).
   mult: x = B' lambda (gluing.c:47-81); mult_transpose: lambda = B x (gluing.c:125-159); in a multi-GPU
   run lambda is replicated and mult_transpose ends with an RCCL all-reduce (replaces PetscSFReduce :144-147). */
typedef struct pmh_gluing_s *pmh_gluing;
int pmh_gluing_create(pmh_ctx ctx, int n_x, int n_lambda, int n_leaves, const int *leaves_row, const int *leaves_root, const double *leaves_sign, pmh_gluing *B);
int pmh_gluing_destroy(pmh_gluing B);
int pmh_gluing_mult(pmh_gluing B, const double *lambda, double *x);
int pmh_gluing_mult_transpose(pmh_gluing B, const double *x, double *lambda);
int pmh_gluing_mult_add(pmh_gluing B, const double *lambda, const double *x1, double *x);                 /* MatMultAdd_Gluing gluing.c:85-123 */
int pmh_gluing_mult_transpose_add(pmh_gluing B, const double *x, const double *lambda1, double *lambda); /* MatMultTransposeAdd_Gluing :163-199 */

/* MATEXTENSION (src/mat/impls/extension/extension.c, the reference's DEFAULT gluing matrix type, qpfeti.c:825-831):
   TA = scatter(ris) * A * gather(cis) with a condensed local CSR A (n_ris x n_cis).
   mult (extension.c:476-489):           r = 0; r[ris] += A * c[cis]
   mult_transpose (extension.c:510-523): c = 0; c[cis] += A' * r[ris]
   ris / cis are host index arrays (each without repeats: they are index sets); n_r, n_c are the lengths of r and c. */
typedef struct pmh_extension_s *pmh_extension;
int pmh_extension_create(pmh_ctx ctx, int n_r, int n_c, pmh_csr A, const int *ris, const int *cis, pmh_extension *TA);
int pmh_extension_destroy(pmh_extension TA);
int pmh_extension_mult(pmh_extension TA, const double *c, double *r);
int pmh_extension_mult_transpose(pmh_extension TA, const double *r, double *c);
int pmh_extension_mult_add(pmh_extension TA, const double *c, const double *r1, double *r);           /* MatMultAdd_Extension extension.c:493-506 */
int pmh_extension_mult_transpose_add(pmh_extension TA, const double *r, const double *c1, double *c); /* MatMultTransposeAdd_Extension :527-540 */

/* MATBLOCKDIAG (src/mat/impls/blockdiag/matblockdiag.c:190-201): the rank's sequential blocks.
   Several subdomains per GPU (BASELINE configs[3]) are stored as ONE concatenated CSR + block offsets. */
typedef struct pmh_blockdiag_s *pmh_blockdiag;
int pmh_blockdiag_create(pmh_ctx ctx, int nblocks, const int *block_rowstart /* nblocks+1 */, pmh_csr Kcat, pmh_blockdiag *K);
int pmh_blockdiag_destroy(pmh_blockdiag K);
int pmh_blockdiag_mult(pmh_blockdiag K, const double *x, double *y);
int pmh_blockdiag_mult_transpose(pmh_blockdiag K, const double *x, double *y);                        /* matblockdiag.c:205-216 */
int pmh_blockdiag_mult_add(pmh_blockdiag K, const double *x, const double *y1, double *y);            /* :220-233, y1 may be y */
int pmh_blockdiag_mult_transpose_add(pmh_blockdiag K, const double *x, const double *y1, double *y);  /* :237-250 */
/* MatMult_BlockDiag on a 3x3-block device copy (the role MATSEQBAIJ bs = 3 plays for 3-dof elasticity blocks: 8.44 instead of 12 bytes per non-zero).
 * share != 0: congruent blocks (checked entry by entry) share ONE device copy -- the product then reads most of K from the XCDs' L2; share == 0: one copy per block,
 * every byte streamed from HBM.  PMH_ERR_SUP if K has no 3x3 block structure.  The transpose / add forms stay on the CSR kernel. */
int pmh_blockdiag_enable_bsr3(pmh_blockdiag K, int share);
/* HIP-event pairs around the launches of pmh_blockdiag_mult.  csr_bytes = 12 nnz + 20 n (SURVEY 8d's figure of the product); hbm_bytes = what the kernel in use has to
 * move from HBM per launch (its stored format; a shared copy once); device_copies = matrix copies on the device (1 when shared, else nblocks). */
int pmh_blockdiag_timing_enable(pmh_blockdiag K, int max_launches);
int pmh_blockdiag_timing_get(pmh_blockdiag K, int *launches, double *total_ms, double *csr_bytes, double *hbm_bytes, int *device_copies);

/* MATINV apply (src/mat/impls/inv/matinv.c:734-743) on the iterative path the reference takes for a
   non-factorisable inner matrix (KSPCG + PCNONE/PCJACOBI per block, matinv.c:535-540): block-wise
   (regularised) CG, every block with its own scalars.  rtol/max_it as KSP; regularisation is the
   caller's (MatRegularize is set-up code). */
typedef struct pmh_matinv_s *pmh_matinv;
int pmh_matinv_create(pmh_blockdiag K, double rtol, double atol, int max_it, int jacobi, pmh_matinv *Kplus);
int pmh_matinv_destroy(pmh_matinv Kplus);
/* MatInvSetNullSpace + Moore-Penrose wrapping P_R K^- P_R (QPTDualize -qpt_dualize_Kplus_mp, qptransform.c:1006-1062).
   R_host: kdim (<= 8) columns of length n, column-major; rows of block b hold that block's orthonormal kernel basis */
int pmh_matinv_set_nullspace(pmh_matinv Kplus, int kdim, const double *R_host);
int pmh_matinv_mult(pmh_matinv Kplus, const double *f, double *u);
/* -qpt_dualize_Kplus_left (QPTDualize qptransform.c:997-1062): K^+ := K^- P_R, what the reference takes when it had to compute the kernel itself.  K^- = the solve of a
   factorisation with null-pivot detection: the fixing dofs (ascending local indices; identity rows / columns in the K given to pmh_matinv_create) carry 0 and their
   equations are dropped.  Needs pmh_matinv_set_nullspace; the result is not projected.  nfix = 0: back to P_R K^- P_R. */
int pmh_matinv_set_left_inverse(pmh_matinv Kplus, int nfix, const int *fix_dofs_host);
/* DEVIATION from the reference, which factorises (matinv.c:481-580) and has no such case: a block whose load lies in the kernel of K_b altogether leaves the block CG only the
 * rounding residue of P_R f_b, which is not in the range of the singular K_b.  ||P_R f_b|| <= c eps ||f_b|| (default c = 64): the block's image is taken as zero (what the
 * Moore-Penrose inverse gives for a load in the kernel); c = 0 switches the rule off.  No other block's threshold is touched. */
int pmh_matinv_set_kernel_load_tolerance(pmh_matinv Kplus, double c);
int pmh_matinv_last_iterations(pmh_matinv Kplus, int *max_block_its, long long *total_spmv);

/* MatRegularize (src/mat/interface/permonmatregularize.c:198-287), the set-up step of the reference's default FETI path
   (-regularize 1 -> MAT_REG_EXPLICIT, qptransform.c:2215,2231; MATINV then factors / iterates on K_reg, matinv.c:449-459).
   Host routines (they run once per block on host CSR / dense R; the per-iteration work stays in pmh_matinv_mult):
   _pivots = MatRegularize_GetPivots_Private (:6-116): the d "fixing" DOFs picked from the p x d column-major kernel basis
             R_loc by complete pivoting from the last column backwards -- index bookkeeping, reproduced exactly;
   _Q      = MatRegularize_GetRegularization_Private (:118-160): RI (RI'RI)^{-1} RI' filtered at 10 eps (d x d row-major);
   _csr    = K_reg = K + rho (rho Q) on the union pattern (rho enters twice, :256,265, kept); rho is the caller's
             pmh_op_max_eigenvalue(K, 1.0, 20, ...) (:254).  Output arrays hold rowptr[n] + d*d entries. */
int pmh_mat_regularize_pivots(int p, int d, const double *R_host, int *pivots_out /* d, ascending */);
int pmh_mat_regularization_Q(int p, int d, const double *R_host, const int *pivots, double *Q_out, int *keep_out);
int pmh_mat_regularize_csr(int n, const int *rowptr, const int *col, const double *val, int d, const double *R_host, double rho, int *pivots_out, int *rowptr_out, int *col_out,
                           double *val_out, long long *nnz_out);

/* QPFetiGetBgtSF (src/qp/impls/feti/qpfeti.c:465-925): the signed gluing matrix of a decomposition from the subdomains' local-to-
   global dof maps (concatenated; l2g_start[nsub+1]).  type 0 nonred / 1 full / 2 orth (FetiGluingType), scale = -SCALE_ON
   (qpfeti.c:757-758), exclude = sorted global dofs left out (-feti_gluing_exclude_dirichlet).  Copies are ordered by subdomain
   index, links by ascending global dof; the leaves come out grouped by link in the summation order of MatMultTranspose_Gluing and
   feed pmh_gluing_create directly (leaves_row = position in the concatenated local numbering).  Host routine (integer set-up,
   runs once).  leaves_* NULL: counts only. */
int pmh_feti_gluing_from_l2g(int nsub, const int *l2g_start, const int *l2g, int type, int scale, int n_exclude, const int *exclude, int *n_lambda, int *n_leaves, int *leaves_row,
                             int *leaves_root, double *leaves_val);

/* F = B K^+ B' (QPTDualize qptransform.c:1103-1128; MatCreateProd matprod.c:42-48) */
int pmh_op_create_feti_dual(pmh_gluing B, pmh_matinv Kplus, pmh_op *F);
/* the applications of F since its creation, through either K^+ (what the dual-space chain serves from its kept intermediates is not one); PMH_ERR_ARG for another operator */
int pmh_feti_dual_applies(pmh_op F, long long *n);
/* PCApply_Dual lumped: y = B K B' x (src/pc/impls/dual/pcdual.c:63-78) */
int pmh_pc_dual_lumped_apply(pmh_gluing B, pmh_blockdiag K, const double *x, double *y);

/* ---- explicit local dual operators: the exact K^+ path of F ------------------------------------------------
 * The reference forms an inverse explicitly column by column with its inner KSP (MatInvExplicitly_Inv, src/mat/impls/inv/
 * matinv.c:670-730, _Private :640-665: one KSPSolve per column of the identity); it applies K^+ inside F = B K^+ B'
 * (qptransform.c:1103-1128) by a per-block factorisation (matinv.c:435-590).  pmh_fexplicit is that explicit inverse restricted
 * to what F can see: for every block b of the rank the dense symmetric W_b = (K_b^+)[Gamma_b, Gamma_b], Gamma_b = the primal
 * dofs of the block that B touches.  F lambda = Bhat blockdiag(W_b) Bhat' lambda: two CSR launches + ONE dense fp64 GEMV that
 * streams 8 n_Gamma_b^2 bytes per block (HBM roofline; SURVEY 8d "dense path"), instead of an inner Krylov solve.
 * _assemble: the columns come from K^+ applications of `solver`, a MATINV whose nslots blocks are solved at once, one unit
 * right-hand side each, at tolerance rtol (1e-12: F exact to that).  block_class[b] / slot_class[s] name classes of identical
 * matrices (pmh_csr_block_classes): blocks of one class share their columns and any slot of the class may produce them; NULL, NULL
 * = slot s solves for block s (solver = the operator's own K^+).  Set-up cost: one K^+ application per
 * ceil(|union of the class's Gamma| / slots of the class). */
typedef struct pmh_fexplicit_s *pmh_fexplicit;
#define PMH_FX_FULL 0 /* W_b as a full row-major matrix: one GEMV, 8 n^2 bytes per block and apply */
#define PMH_FX_SYM 1  /* W_b = W_b' kept as its lower block-triangle (bands of 32 rows): a deterministic two-launch SYMV, 4 n^2 bytes */
#define PMH_FX_CLASS 2 /* pmh_fexplicit_create_shared: congruent blocks share ONE full matrix W_c = (K^+)[U_c, U_c] per class (U_c = union of their
                          Gamma_b) applied to the blocks' vectors together, 8 right-hand sides per pass: 8 n_c^2 bytes for the whole class */
int pmh_fexplicit_create(pmh_gluing B, pmh_blockdiag K, int storage, pmh_fexplicit *E); /* finds Gamma_b, allocates the dense blocks (zero) */
#define PMH_FX_CLASS_SYM 3 /* pmh_fexplicit_create_shared_sym: the same W_c kept as its lower block-triangle in 16 x 16 tiles (4 n_c^2 bytes for the
                              whole class); both products of a tile with the 8 right-hand sides run on the fp64 matrix instruction (4x4x4_4b) */
#define PMH_FX_CLASS_ORBIT 4 /* pmh_fexplicit_create_shared_orbit: W_c is invariant under the class's symmetries (pmh_fexplicit_set_class_symmetry /
                                _set_box_symmetry, REQUIRED before the assembly), so only the rows of the orbit representatives are kept (a cube: 1 / 48 of
                                the rows) and F's dense part becomes a GEMM over (representatives) x (operations x 8 right-hand sides) on the fp64 matrix
                                instruction: 48 flop per stored byte instead of 4 -- compute-bound instead of HBM-bound */
int pmh_fexplicit_create_shared(pmh_gluing B, pmh_blockdiag K, const int *block_class, pmh_fexplicit *E); /* storage PMH_FX_CLASS */
int pmh_fexplicit_create_shared_orbit(pmh_gluing B, pmh_blockdiag K, const int *block_class, pmh_fexplicit *E); /* storage PMH_FX_CLASS_ORBIT */
/* the same with the touched set of class c extended by the block-relative dofs extra_rel[extra_ptr[c] .. extra_ptr[c + 1]) -- e.g. its closure under the block's symmetries
   (pmh_box_symmetry_closure), which lets a class of ONE box-shaped block (non-congruent decompositions: one material per subdomain) keep all the box's operations */
int pmh_fexplicit_create_shared_orbit_union(pmh_gluing B, pmh_blockdiag K, const int *block_class, const int *extra_ptr, const int *extra_rel, pmh_fexplicit *E);
int pmh_fexplicit_apply_flops(pmh_fexplicit E, double *flops); /* PMH_FX_CLASS_ORBIT: useful flops of the dense apply = (rows of the row tiles) x (the columns their blocks need) x 2 n_c (the roofline of that storage is the fp64 MFMA peak); 0 otherwise */
int pmh_fexplicit_apply_flops_detail(pmh_fexplicit E, double *issued /* padded tiles, what the matrix cores execute */, double *dense /* every (representative, operation, block): the count without the pruning by the blocks' touched dofs */);
int pmh_fexplicit_create_shared_sym(pmh_gluing B, pmh_blockdiag K, const int *block_class, pmh_fexplicit *E); /* storage PMH_FX_CLASS_SYM */
int pmh_fexplicit_destroy(pmh_fexplicit E);
int pmh_fexplicit_sizes(pmh_fexplicit E, int *nblocks, int *n_gamma /* [nblocks] or NULL */, long long *dense_bytes, double *gemv_algorithmic_bytes);
/* several GPUs, congruent blocks: E built over ALL blocks (B = the global gluing, K = the global block structure); this rank
   assembles and applies the 128-row stripes idx = rank (mod size) of the size-ordered list -- an even share of the dense bytes; the
   all-reduce that ends B u completes F lambda (PMH_FX_CLASS: a contiguous range of the rows of W_c; PMH_FX_CLASS_SYM: whole 256-row super
   bands dealt in snake order).  Not for PMH_FX_FULL; before the assembly. */
int pmh_fexplicit_set_stripe(pmh_fexplicit E, int rank, int size);
int pmh_fexplicit_stripe_owner(int nblocks, const int *n_gamma, int size, int *owner_out); /* host: owner rank of every 128-row stripe, block after block */
int pmh_fexplicit_stripe_bytes(int nblocks, const int *n_gamma, int size, double *bytes_per_rank); /* host: dense bytes per rank under that rule */
/* set-up by symmetry (PMH_FX_CLASS_SYM): nsym signed permutations of the class's touched dofs U_c (pmh_fexplicit_class_union: their indices relative to the
   block start, ascending = the row numbering of W_c) under which K_c, hence K_c^+, is invariant -- posmap[g * n_c + c] = position in U_c of the image of the
   c-th touched dof, sign[g * n_c + c] = +-1, operation 0 the identity.  W[g p][g c] = sign_g[p] sign_g[c] W[p][c]: ONE K^+ solve per ORBIT of rows (a cube
   of identical Q1 elasticity elements: the 48 signed coordinate permutations, 48 x fewer set-up solves).  The caller vouches for the invariance; the
   assembly re-solves a batch of symmetry-filled rows directly and fails if they differ.  Before pmh_fexplicit_assemble. */
/* host helper: the signed dof permutations of a box of dims[0] x dims[1] x dims[2] nodes (x fastest, ndof dofs per node; ndof = 3: vector components)
   induced by the signed coordinate permutations that map the box onto itself and leave the block's matrix (CSR rowptr / col / val, n rows; NULL: not
   checked) invariant -- generators checked on nsample rows, the group is their closure (<= 48 operations, 0 = identity).  perm, sign: [48 * n]. */
int pmh_box_symmetries(const int *dims, int ndof, const int *rowptr, const int *col, const double *val, int nsample, int *nsym, int *perm, signed char *sign);
/* the same, and the operations themselves: ops[6 g ...] = (ax[3], fl[3]), new coordinate a = fl[a] * old coordinate ax[a] (NULL: not wanted) */
int pmh_box_symmetries_ops(const int *dims, int ndof, const int *rowptr, const int *col, const double *val, int nsample, int *nsym, int *perm, signed char *sign, int *ops);
/* Host routine (no device): the symmetry-adapted basis of the dofs rel[0 .. n_c) (block-relative, ascending, closed under the box's 48 operations) of a cube.  mult / dim: [10]
   multiplicity and dimension of the irreps A1g A2g Eg T1g T2g A1u A2u Eu T1u T2u; the basis functions are numbered orbit after orbit, irrep after irrep, copy after copy, partner
   after partner; orbit o (of orb_size[o] positions, orb_pos in the same running order) owns as many functions as positions.  Per function: its irrep, the row of its copy in the
   irrep's block W^_i, its partner, the copy's vector v_k (3 doubles) and its values on the orbit's positions (tables[48 row ...]).  PMH_ERR_SUP: no such basis (not all 48). */
int pmh_orbit_basis(const int *dims, int ndof, int n_c, const int *rel, int *norb, int *mult, int *dim, int *orb_size, int *orb_pos, int *row_irrep, int *row_index, int *row_partner,
                    double *row_v, double *tables);
/* whether class cls of a PMH_FX_CLASS_ORBIT operator applies W_c in the symmetry-adapted basis (after the assembly) */
int pmh_fexplicit_orbit_adapted(pmh_fexplicit E, int cls, int *adapted);
/* sorted union of the images of the dofs in_rel under those operations (out_rel: capacity nx ny nz ndof, may be NULL to get the count); host */
int pmh_box_symmetry_closure(const int *dims, int ndof, const int *rowptr, const int *col, const double *val, int n_in, const int *in_rel, int *n_out, int *out_rel, int *nsym);
/* the two together for box-shaped blocks: symmetries of the box checked against the CSR of one block of the class (column indices relative to the block),
   restricted to those that map the class's touched dofs onto themselves, handed to pmh_fexplicit_set_class_symmetry; nsym_used: how many (1 = none) */
int pmh_fexplicit_set_box_symmetry(pmh_fexplicit E, int cls, const int *dims, int ndof, const int *rowptr, const int *col, const double *val, int *nsym_used);
int pmh_fexplicit_class_union(pmh_fexplicit E, int cls, int *n_c, int *urel_out /* [n_c] or NULL */);
int pmh_fexplicit_set_class_symmetry(pmh_fexplicit E, int cls, int nsym, const int *posmap, const signed char *sign);
int pmh_fexplicit_class_sym_plan(int n_c, int size, int *megaband_owner /* [ceil(ceil(n_c / 256) / 4)] or NULL */, double *bytes_per_rank /* [size] or NULL */); /* host: PMH_FX_CLASS_SYM's rule */
int pmh_fexplicit_orbit_row_tile(int n_representatives, int *row_tile /* 128, 120, 112, 104 or 96 */, int *padded_rows); /* host: PMH_FX_CLASS_ORBIT's rule for the row tile of its GEMM */
int pmh_fexplicit_assemble(pmh_fexplicit E, pmh_matinv solver, int nslots, const int *slot_class, const int *block_class, double rtol, int max_it);
/* nslots == 8 x (blocks of the solver): the multi-right-hand-side K^+ (csrc/matinv_mv.hip) solves 8 columns per block and application, slot s = column s % 8 of block s / 8
   (slot_class per slot; PMH_ERR_SUP where that solver does not apply).  pmh_fexplicit_assemble_auto tries exactly that and falls back to one column per block;
   slot_class there names the class of every BLOCK of the solver.  Column-blocked set-up of the reference: MatInvExplicitly_Inv, src/mat/impls/inv/matinv.c:640-730. */
int pmh_fexplicit_assemble_auto(pmh_fexplicit E, pmh_matinv solver, const int *slot_class, const int *block_class, double rtol, int max_it, int *used_multi_rhs /* or NULL */);
int pmh_fexplicit_fill_pattern(pmh_fexplicit E, int byte); /* tuning helper: byte pattern instead of the assembly (not F afterwards) */
int pmh_fexplicit_assemble_stats(pmh_fexplicit E, long long *n_solves, double *seconds);
int pmh_fexplicit_get_block(pmh_fexplicit E, int b, double *W_host /* n_Gamma_b^2 row-major or NULL */, int *gamma_host /* or NULL */);
int pmh_fexplicit_mult(pmh_fexplicit E, const double *lambda, double *y);              /* y = F lambda (MatMult of the product) */
int pmh_fexplicit_compressed_size(pmh_fexplicit E, int *ntot, int *gstart /* [nblocks+1] or NULL */);
int pmh_fexplicit_dense_mult(pmh_fexplicit E, const double *xhat, double *yhat);        /* the dense kernel alone, compressed vectors */
int pmh_fexplicit_timing_enable(pmh_fexplicit E, int max_launches, int stride);         /* HIP-event pairs around the GEMV launches */
int pmh_fexplicit_timing_get(pmh_fexplicit E, int *launches, double *total_ms, double *first_kernel_ms /* SYM: k_fx_symv alone; CLASS_ORBIT: the GEMM kernel alone (total - first = the finishing kernel); or NULL */);
/* PCDUAL dirichlet: y = B S B' x, S = blockdiag(S_b), S_b = K_GG - K_GI K_II^{-1} K_IG the Schur complement of block b on Gamma_b (the dofs of the block
 * that B touches, as pmh_fexplicit_create takes them) against the rest of the block.  The reference's PCApply_Dual (src/pc/impls/dual/pcdual.c:63-78) is
 * y = At' C_bb At x; PCSetUp_Dual (:105-116) fills C_bb = K for `lumped` only -- this is the same apply with C_bb = S, the preconditioner whose condition
 * number stays polylogarithmic in H/h.  Set-up: one Jacobi-PCG solve with K_II per column of every S_b that has an interior (all blocks' columns of one batch in one
 * application of a block CG over blockdiag(K_II,b), tolerance rtol, at most max_it iterations; PMH_ERR_STATE if one does not converge), S_b = K_b[Gamma_b, Gamma_b] for a
 * block without an interior; S_b is stored exactly symmetric ((S_b + S_b') / 2) in a pmh_fexplicit of `storage` PMH_FX_FULL (8 n_Gamma_b^2 bytes) or PMH_FX_SYM (4 n_Gamma_b^2)
 * and every apply is pmh_fexplicit_mult.  Class-shared storage and several GPUs: PMH_ERR_SUP.  K_b symmetric; destroy with pmh_op_destroy.
 * _stats: set-up solves (sum of n_Gamma_b over the blocks with an interior), set-up wall seconds, bytes of the dense storage.  _get_block (tests): S_b as stored,
 * n_Gamma_b^2 row-major, and Gamma_b (rank-local primal dofs), either may be NULL.  _get_explicit: the pmh_fexplicit inside, borrowed (pmh_fexplicit_sizes /
 * pmh_fexplicit_timing_*). */
int pmh_op_create_pc_dual_dirichlet(pmh_gluing B, pmh_blockdiag K, int storage, double rtol, int max_it, pmh_op *op);
int pmh_pc_dual_dirichlet_stats(pmh_op op, long long *n_solves, double *setup_seconds, double *dense_bytes);
int pmh_pc_dual_dirichlet_get_block(pmh_op op, int b, double *S_host, int *gamma_host);
int pmh_pc_dual_dirichlet_get_explicit(pmh_op op, pmh_fexplicit *E);
/* F = B K^+ B' built on this MATINV (pmh_op_create_feti_dual, the FETI chain) applies through E from now on (E built from the
   same B; NULL detaches).  K^+ f for a general f (d = B K^+ f - c, primal recovery) stays on the inner KSP. */
int pmh_matinv_attach_explicit(pmh_matinv Kplus, pmh_fexplicit E);
int pmh_matinv_set_tolerances(pmh_matinv Kplus, double rtol, double atol, int max_it);  /* KSPSetTolerances of MatInvGetKSP's KSP */
int pmh_matinv_get_tolerances(pmh_matinv Kplus, double *rtol, double *atol, int *max_it);
/* classes of bit-identical diagonal blocks of a block-diagonal host CSR (congruent subdomains): block_class[b] in [0, nclasses) */
int pmh_csr_block_classes(int nblocks, const int *block_rowstart, const int *rowptr, const int *col, const double *val, int *block_class, int *nclasses);

/* ---- QP transform chain of the (T)FETI path, data part (src/qp/interface/qptransform.c) -------------------------------
   QPTDualize (:1102-1174: F = B K^+ B', d = B K^+ f - c) -> QPTHomogenizeEq (:437-527: lambda~ = G'(GG')^{-1} e,
   b_bar = d - F lambda~, lb <- lb - lambda~) -> QPTEnforceEqByProjector (:215-316: A = P F P with a box, P F without;
   b = P b_bar).  f: n_x, c / lb: n_lambda (lb NULL = no box, -inf on equality rows otherwise), e: rows of G; pf NULL = no
   equality constraint (no floating subdomain).  The handles stay owned by the caller, the chain owns what it creates. */
typedef struct pmh_feti_chain_s *pmh_feti_chain;
int pmh_qpt_feti_chain_create(pmh_gluing B, pmh_matinv Kplus, const double *f, const double *c, pmh_qppf pf, const double *e, const double *lb, pmh_feti_chain *ch);
int pmh_qpt_feti_chain_get(pmh_feti_chain ch, pmh_op *F, pmh_op *A, double **d, double **b_bar, double **b, double **lb_new, double **lambda_tilde); /* borrowed */
/* QPTHomogenizeEqPostSolve_Private (:423-431) + the operator part of QPTDualizePostSolve_Private (:783-833):
   lambda = lambda_child + lambda~; u0 = K^+(f - B' lambda); r = F lambda - d (u0, r optional) */
int pmh_qpt_feti_chain_post_solve(pmh_feti_chain ch, const double *lambda_child, double *lambda, double *u0, double *r);
int pmh_qpt_feti_chain_destroy(pmh_feti_chain ch);
/* the numbers of -qp_chain_view_kkt (QPViewKKT qp.c:245-369 on every QP of the chain, qpchain.c:247-268) for the QPs this chain object stands for; linear chain (no dual box).
 * K: the block-diagonal stiffness of the primal QP; x_child: the solved vector of the last QP; lambda = x_child + lambda~; u: the recovered primal solution */
typedef struct {
  int    has_coarse;                             /* the projected and the homogenised QP exist (floating subdomains) */
  double proj_r, proj_normb;                     /* ||P F x - P b_bar||, ||P b_bar|| */
  double hom_r, hom_be, hom_normb;               /* ||F x - b_bar + (B'lambda)|| (0 by construction of the missing multiplier), ||G x||, ||b_bar|| */
  double dual_r, dual_be, dual_normb;            /* ||F lambda - d + (B'lambda)||, ||G lambda - e||, ||d|| */
  double prim_r, prim_be, prim_normb;            /* ||K u - f + B' lambda||, ||B u||, ||f|| */
  double prim_r_zeroed_operator;                 /* ||B' lambda - f||: the same line once QPTPostSolve_QPTMatISToBlockDiag has left K zeroed (-qpt_matis_to_diag_norm with Dirichlet by B) */
} pmh_feti_chain_kkt;
int pmh_qpt_feti_chain_kkt(pmh_feti_chain chain, pmh_blockdiag K, const double *x_child, const double *lambda, const double *u, pmh_feti_chain_kkt *out);

/* ---- dense-row SVM dual Hessian (BASELINE configs[4]) ---------------------------------------------------- */
/* H = diag(y) X X' diag(y), X: n_local x d row-major in HBM (d <= 256), applied as two GEMV passes; with a
   communicator the samples are sharded by rows and w = X'(y o a) is all-reduced (d doubles) between the passes */
int pmh_op_create_svm_dual(pmh_ctx ctx, int n_local, int d, const double *X_dev, const double *y_dev, pmh_op *op);
/* The same operator over samples stored in float32 (X_dev: n_local x d floats, row-major, borrowed): half the device memory and half the traffic of X per pass.
   Only the storage of X changes: a float enters the arithmetic as (double)x, which is exact; w, every n-vector, every partial sum and the all-reduce stay fp64.
   Any d but 64: the kernels of the fp64 operator with another load, bit for bit what pmh_op_create_svm_dual gives on the widened samples.  d = 64: a layout
   of its own on 16-byte loads (four rows per wave-instruction), whose summation order is fixed (no float atomics; two runs give the same bits) but is not the fp64
   layout's: results agree with the fp64 operator's to rounding.  Terms, diagonal, subsets, labels, the paired passes and a communicator work as on the fp64
   operator; same limits (d <= 256) */
int pmh_op_create_svm_dual_f32(pmh_ctx ctx, int n_local, int d, const float *X_dev, const double *y_dev, pmh_op *op);
/* how many times the operator has streamed X since it was created (2 per plain application; inside pmh_mpgp_solve on one GPU with d = 64 the second pass of an
   application also does the first pass of the next one wherever the MPGP step allows it -- svm.hip, "paired passes" -- so a run of expansion steps costs 2 passes
   per step instead of 4): what a bandwidth figure for this operator has to be computed from */
int pmh_op_svm_dual_passes(pmh_op op, long long *passes);
/* the augmented Hessian H + shift I + sigma y y' (shift, sigma >= 0; both 0: the plain operator, its kernels and its bits).  shift = 1/C is the L2-loss dual's
   Hessian; sigma y y' is what penalising the bias equality y'a = 0 adds.  One more column sum, s = sum_i y_i a_i, travels with the d of w: no extra pass over X,
   and every fused epilogue of the plain operator carries both terms */
int pmh_op_svm_dual_set_terms(pmh_op op, double shift, double sigma);
/* H + diag(diag) + sigma y y': a diagonal in place of the scalar shift (the L2-loss dual with a penalty per sample: diag_i = 1 / C_i).  diag_dev: n_local doubles
   on the device, borrowed until it is replaced or the operator destroyed; NULL: off.  Dense rows of any admitted d and CSR.  Pass 2 reads diag_i where it
   reads a_i and y_i: 8 more bytes per sample, no extra launch, and the paired passes, the folded one-row equality and the ||B u|| rider stay as with a shift.
   A diagonal and a non-zero shift exclude each other: whichever call arrives second while the other term is on is PMH_ERR_ARG.  Prepared sums of the paired
   passes are dropped, as by pmh_op_svm_dual_set_terms */
int pmh_op_svm_dual_set_diag(pmh_op op, const double *diag_dev /* n_local doubles, borrowed; NULL: off */);
/* The same operator for samples in CSR (X: n_local x d, any d >= 1, column indices ascending inside a row; y in {-1, +1}); X and y_dev are borrowed and must
   stay unchanged.  Two sweeps over the stored entries per application, the work divided by entries, no float atomics: the same input gives the same bits
   (svm_csr.hip).  Creation builds a column-ordered device copy of X: 12 (nnz + n_local) bytes beside X.  Unsorted column indices and nnz + n_local >= 2^31 are
   PMH_ERR_ARG.  pmh_op_svm_dual_set_terms and pmh_op_svm_dual_passes apply (a pass = one sweep over all stored entries); no fused MPGP epilogues */
int pmh_op_create_svm_dual_csr(pmh_ctx ctx, pmh_csr X, const double *y_dev, pmh_op *op);
/* New labels on a created operator (dense rows or CSR): y_dev, n_local doubles of +-1, borrowed from now on in place of the old ones.  y_dev MAY be the buffer
   the operator borrows already, with new contents: the operator reads nothing of the old labels from the caller's memory.  Dense rows: the pointer is swapped
   and prepared sums of the paired passes are dropped, as by pmh_op_svm_dual_set_terms.  CSR: the column-ordered copy (12 (nnz + n_local) bytes) is re-signed in
   place, every stored value times y_i(old) y_i(new) = +-1 from the signs the operator keeps itself -- 8 n_local bytes more beside the copy -- so the copy
   equals, bit for bit, the one a fresh operator builds.  Terms and diagonal stay as set */
int pmh_op_svm_dual_set_labels(pmh_op op, const double *y_dev /* n_local doubles, borrowed */);
/* A sample subset S on a created operator (dense rows or CSR): H_S = M (H + D) M with M = diag(m), D the scalar shift or the diagonal, i.e.
     out_i = m_i [ y_i (x_i . w) + sigma s y_i + D_i v_i ],  w = sum_{j in S} y_j v_j x_j,  s = sum_{j in S} y_j v_j.
   m_dev: n_local doubles on the device, each exactly 0 or 1, read during the call only (the operator keeps a copy and the masked labels m o y: 16 n_local bytes);
   NULL: all samples, the plain operator again.  Any other entry (a NaN is one) is PMH_ERR_ARG with the count, an all-zero mask (over all ranks) too; a refused
   mask changes nothing.  Held-out rows of the result are exactly 0, shift or diagonal included; held-out entries of v have no effect whatever they hold.  The
   subset survives pmh_op_svm_dual_set_labels, _set_terms and _set_diag; prepared sums of the paired passes are dropped.  Dense rows: a held-out row of X is not
   read at all (the kernels' SUB instances read the masked label first), in both passes, the paired passes and the ||B u|| rider, which all stay in use; CSR:
   every stored entry is still swept (no row skipping), one n-vector kernel masks the operand before pass 1 */
int pmh_op_svm_dual_set_subset(pmh_op op, const double *m_dev /* n_local doubles of 0 / 1, or NULL = all */);

/* ---- the dual Hessian of epsilon-insensitive regression (svr.hip) ---------------------------------------------------------------------------------------------
 * The classification dual on the doubled samples [X; X] with labels [+1; -1], X kept ONCE.  The operator acts on 2 n_local doubles u = [p; q]:
 *   s_i = p_i - q_i,  w = X's,  S = sum_i s_i,
 *   out_p[i] =   x_i . w  + sigma S + D_i p_i
 *   out_q[i] = -(x_i . w) - sigma S + D_i q_i,      D the scalar shift or the diagonal (n_local doubles, used for both halves).
 * Dense rows (fp64 or float32, d <= 256, X borrowed and never copied): a product streams X twice in three launches -- pass 1 reads p_i and q_i where the
 * classification kernel reads y_i a_i, the column sums, pass 2 writes both halves of row i from the one dot product; no n-vector s or X w goes through memory.
 * Fixed summation orders, no float atomics: two products give the same bits.  float32 with d != 64: bit for bit the fp64 operator on the widened samples.
 * CSR (any d): the entry-balanced sweeps of the classification operator over X with all labels +1 (one column-ordered copy, 12 (nnz + n_local) bytes), one
 * n-vector kernel before pass 1 (p - q) and one after pass 2 (the two halves).  Device memory beside X, CSR: that copy, the sweeps' tables and 6 n-vectors of
 * doubles (the labels of both orderings 2, p - q 1, X w 1, the labels [+1; -1] of the doubled problem 2); dense: the last 2 only.
 * With a communicator the samples are sharded by rows and w (d doubles, d + 1 with sigma) is all-reduced between the passes (kept, not tested on more than one
 * GPU).  Under pmh_op_create_penalized with a one-row projector whose row is a multiple of [1; -1] the penalty is absorbed as the rank-one term (as the
 * classification operator does).  No fused MPGP epilogues (MPGP takes its unfused path), no new labels.
 * set_terms / set_diag: the rules of pmh_op_svm_dual_set_terms / _set_diag (shift, sigma >= 0; a diagonal and a non-zero shift exclude each other). */
int pmh_op_create_svr_dual(pmh_ctx ctx, int n_local, int d, const double *X_dev, pmh_op *op);
int pmh_op_create_svr_dual_f32(pmh_ctx ctx, int n_local, int d, const float *X_dev, pmh_op *op);
int pmh_op_create_svr_dual_csr(pmh_ctx ctx, pmh_csr X, pmh_op *op);
int pmh_op_svr_dual_set_terms(pmh_op op, double shift, double sigma);
int pmh_op_svr_dual_set_diag(pmh_op op, const double *diag_dev /* n_local doubles, borrowed, used for both halves; NULL: off */);
int pmh_op_svr_dual_passes(pmh_op op, long long *passes); /* passes over X so far: 2 per product */
/* A sample subset S on a created regression operator (dense rows or CSR).  m_dev: n_local doubles on the device, each exactly 0 or 1, read during the call only
   (the operator keeps [m; -m], the masked labels of the doubled problem: 16 n_local bytes); NULL: all samples, the plain operator again.  With M^ = diag([m; m])
   and e^ = [m; -m]:
     out = M^ [Q + D, -Q; -Q, Q + D] M^ u + sigma (e^'u) e^.
   The mask's rules are pmh_op_svm_dual_set_subset's, checked by the same function: any other entry (a NaN is one) is PMH_ERR_ARG with the count, an all-zero
   mask (over all ranks) too; a refused mask changes nothing.  Rows outside S are exactly +0 in both halves; entries of u outside S are selected away, not
   multiplied by 0: whatever they hold (a NaN, 1e300) changes no bit of the result.  The subset survives _set_terms and _set_diag.  Dense rows: the SUB = 1
   instances of the four kernels read the mask first -- d = 64: of the 8 (float32: 16) rows a wave has in flight in one coalesced load and a ballot -- and issue
   no load of a held-out row of X in either pass; a product is still three launches and two counted passes.  CSR: every stored entry is still swept (no row
   skipping) and there is no second column-ordered copy: the inner classification operator takes the mask, n-vector kernels do the rest.
   pmh_op_svm_dual_set_subset goes on refusing a regression operator */
int pmh_op_svr_dual_set_subset(pmh_op op, const double *m_dev /* n_local doubles of 0 / 1, or NULL = all */);

/* ---- QPS SMALXE (src/qps/impls/smalxe/smalxe.c) -------------------------------------------------------- */
typedef struct {
  double rtol, atol, divtol;
  int    max_it;             /* outer, default 100 (smalxe.c:1203) */
  double M1_user;  int M1_direct;  double M1_update;
  double rtol_E;
  double rho_user; int rho_direct; double rho_update, rho_update_late;
  double eta_user; int eta_direct;
  double update_threshold;
  double maxeig, maxeig_tol; int maxeig_iter;
  int    inject_maxeig, inject_maxeig_set;
  int    inner_iter_min, inner_no_gtol_stop;
  /* ||Bu|| update (smalxe.c:878-886): be_implicit = BE has no mult slot, only B'B is available -> QPSSMALXEUpdateNormBu_SMALXEON
     (:265-285, ||Bu|| = sqrt(u'B'Bu), BtBu reused by the lambda update), with lag_enabled (-qps_smalxe_norm_update_lag) the lagged
     variant (:289-370; offset / Jstart / Jstep / Jend / lower / upper as :757-762, defaults :1190-1200) */
  int    be_implicit, lag_enabled, lag_offset, lag_start, lag_step, lag_end;
  double lag_lower, lag_upper;
  int    knoll;              /* -qps_smalxe_knoll (smalxe.c:764,938-943): u0 = P b */
  pmh_mpgp_opts inner;       /* inner MPGP (prefix smalxe_) */
} pmh_smalxe_opts;

typedef struct {
  int    iteration, reason, inner_iter_accu, state;
  int    M1_hits, eta_hits, M1_updates, rho_updates;
  double M1, rho, eta, normBu, enorm, rnorm, maxeig;
  pmh_mpgp_stats inner;
} pmh_smalxe_stats;

typedef struct pmh_smalxe_s *pmh_smalxe;
int pmh_smalxe_default_opts(pmh_smalxe_opts *o);
/* QPSSetUp_SMALXE smalxe.c:772-888: A (outer Hessian, e.g. P F P), b, u, box, pf with BE = G, cE = 0 */
int pmh_smalxe_create(pmh_ctx ctx, pmh_op A, const double *b, double *u, const double *lb, const double *ub, pmh_qppf pf, const pmh_smalxe_opts *o, pmh_smalxe *s);
int pmh_smalxe_destroy(pmh_smalxe s);
int pmh_smalxe_solve(pmh_smalxe s);                                  /* QPSSolve_SMALXE smalxe.c:893-997 */
/* Extension, off by default: carry A_rho u from the last gradient of an inner solve into the Lagrangian (smalxe.c:982 forms it by QPComputeObjective's own MatMult)
   and into the first gradient of the next inner solve (mpgp.c:500 starts every solve with MatMult) -- g' = g + rho_new B'B u, B'B u being at hand for the multiplier
   update: two operator applications less per outer iteration, the same iterates up to the rounding of g's recurrence over the CG steps of the inner solve.  The
   number of Hessian multiplications reported then differs from the reference's for the same solve. */
int pmh_smalxe_set_reuse_products(pmh_smalxe s, int on);
int pmh_smalxe_get_stats(pmh_smalxe s, pmh_smalxe_stats *st);
int pmh_smalxe_reset(pmh_smalxe s);                                  /* QPSReset: the state machine of the inner convergence test back to 1 (a solve from a fresh initial guess) */
/* One-shot: the next pmh_smalxe_solve starts from the caller's pair (u, B'mu = Btmu0) where it otherwise zeroes B'mu; the solve after that one starts from
   zero again.  On such a solve: the Knoll start (-qps_smalxe_knoll) is not applied, the caller's u being the start; u is projected onto the box and the pair is
   put to the outer criterion before anything moves -- rnorm = max(|B u| / rtol_E, |gP|), gP the projected gradient of A u - b + B'mu, one product with A -- and
   where it holds the solve returns with 0 outer and 0 inner iterations, u and B'mu the caller's; otherwise the first inner problem is posed with B'mu as given
   (the update B'mu += rho B'B u every later outer iteration begins with is not made from the caller's u, which no inner solve has produced).  M1, rho and the
   state machine are reset exactly as in any solve.  Btmu0_dev: n doubles on the device, copied (it may be the solver's own B'mu of pmh_smalxe_get_penalized,
   filled in place); NULL: zero, as without the call */
int pmh_smalxe_set_initial_multiplier(pmh_smalxe s, const double *Btmu0_dev /* n, copied; NULL: zero */);
int pmh_smalxe_set_inner_max_it(pmh_smalxe s, int max_it);           /* the inner QPS's iteration limit, summed over the outer iterations (smalxe.c:626-631: DIVERGED_ITS / outer BREAKDOWN beyond it) */
int pmh_smalxe_get_inner_max_it(pmh_smalxe s, int *max_it);
int pmh_smalxe_get_solution(pmh_smalxe s, pmh_ctx *ctx, double **u, int *n); /* QPGetSolutionVector: the caller's device vector (+ context, length); any pointer may be NULL */
int pmh_smalxe_get_penalized(pmh_smalxe s, pmh_op *A_rho, double **b_inner, double **Bt_mu); /* the penalised child QP (A + rho B'B, b - B'mu) and B'mu (borrowed; any may be NULL) */
int pmh_smalxe_get_inner(pmh_smalxe s, pmh_mpgp *inner);             /* QPSSMALXEGetInnerQPS smalxe.c:492-507 (borrowed) */

/* ---- options front end (QPSSetFromOptions qps.c:860-900, _MPGP mpgp.c:712-745, _SMALXE smalxe.c:696-766) ----------
 * The reference is configured from PETSc's options database; this parses the same keys out of a PETSc-style option string
 * (command line / permonrc contents) into the option structs, with the argument checks of the reference's setters.
 * prefix: options prefix of the QPS object ("" for the top solver); SMALXE's inner MPGP reads <prefix>smalxe_qps_* (smalxe.c:500-502).
 * unknown: optional buffer for the keys nobody consumed (PETSc's -options_left), space separated. */
typedef struct {
  char   type[16];           /* -qps_type: "mpgp" | "smalxe" | "pcpg" | "ksp"; "" = QPSSetDefaultType decides (qps.c:422-455) */
  double rtol, atol, divtol; /* -qps_rtol / -qps_atol / -qps_divtol (QPSSetTolerances qps.c:905-930) */
  int    max_it, max_it_set; /* -qps_max_it */
  int    monitor, monitor_cost, view, view_convergence, auto_post_solve;
} pmh_qps_opts;
int pmh_qps_default_opts(pmh_qps_opts *q);
int pmh_qps_set_from_options(const char *options, const char *prefix, pmh_qps_opts *q, pmh_mpgp_opts *m, pmh_smalxe_opts *s /* or NULL */, char *unknown, int unknown_cap);

/* ---- SVM front end: train, model, predict (the role of PermonSVM, a separate repository the reference's README names; its sources were not available when
 * this was written, so the option names below are this library's own and no compatibility with PermonSVM's is claimed) ----------------------------------------
 * Dual problems, H = diag(y) X X' diag(y), X n x d row-major on the device (one sample per row), y in {-1, +1}:
 *   L1: min 1/2 a'Ha - 1'a,          0 <= a <= C      (primal 1/2 |w|^2 + C sum xi)
 *   L2: min 1/2 a'(H + I/C)a - 1'a,  0 <= a           (primal 1/2 |w|^2 + C/2 sum xi^2)
 *   bias: additionally y'a = 0, posed as (y / sqrt(n))'a = 0 (a row of unit length).
 * Without bias the QP goes to MPGP; with bias to SMALXE over a one-row projector (pmh_qppf_create_onerow), whose penalty rho B'B the SVM operator absorbs as its
 * rank-one term: the same passes over X per inner iteration as without bias.
 * Model: w = X'(y o a); b = mean over the free support vectors of (y_i - x_i . w), free meaning astol < a_i and, for L1, a_i < C - astol (astol: the inner
 * MPGP's, 10 eps).  If no sample is free, b is taken from the equality's Lagrange multiplier: with the Lagrangian 1/2 a'Ha - 1'a + mu (y / sqrt(n))'a that SMALXE
 * works on (it keeps B'mu = mu y / sqrt(n)), stationarity in a free sample reads y_i - x_i . w = mu / sqrt(n), so b = mu / sqrt(n).  Both are reported
 * (pmh_svm_stats::b_free, ::b_multiplier); they agree to the tolerance of the solve.  Decision function: x . w + b, label +1 where it is >= 0, else -1. */
enum { PMH_SVM_LOSS_L1 = 0, PMH_SVM_LOSS_L2 = 1 };
typedef struct {
  int             loss_type;  /* -svm_loss_type L1 | L2 */
  double          C;          /* -svm_C, > 0 */
  int             bias;       /* -svm_bias 0 | 1 */
  pmh_qps_opts    qps;        /* -qps_rtol / _atol / _divtol / _max_it: the tolerances of the solver that trains (MPGP, or the outer SMALXE) */
  pmh_mpgp_opts   mpgp;       /* -qps_mpgp_*: the solver without bias */
  pmh_smalxe_opts smalxe;     /* -qps_smalxe_* and -smalxe_qps_*: the solver with bias and its inner MPGP */
} pmh_svm_opts;
typedef struct {
  int       reason;                            /* converged reason of the training solve */
  int       outer_iterations, inner_iterations; /* SMALXE's outer and accumulated inner iterations (no bias: 0 and MPGP's iterations) */
  int       nmv, ncg, nexp, nprop;             /* Hessian multiplications and step types of the (inner) MPGP */
  long long passes_X;                          /* passes over X of the solve (pmh_op_svm_dual_passes before and after) */
  long long n_sv, n_free_sv;                   /* support vectors (a_i > astol), free ones */
  double    yTalpha;                           /* y'a of the returned dual solution */
  double    b, b_free, b_multiplier;           /* the bias returned, the mean over the free support vectors (NaN: none), the multiplier's value */
  double    rho, normBu, rnorm;                /* SMALXE's final penalty, |B a| and residual norm (no bias: 0, 0, MPGP's) */
} pmh_svm_stats;
typedef struct pmh_svm_s *pmh_svm;
int pmh_svm_default_opts(pmh_svm_opts *o);
/* -svm_loss_type, -svm_C, -svm_bias here; everything else through pmh_qps_set_from_options with the empty prefix.  An unknown loss type is PMH_ERR_ARG with a message */
int pmh_svm_set_from_options(const char *options, pmh_svm_opts *o, char *unknown, int unknown_cap);
/* X_dev (n_local x d, d <= 256) and y_dev are borrowed: the caller keeps them alive and unchanged.  Under a communicator the samples are sharded by rows */
int pmh_svm_create(pmh_ctx ctx, int n_local, int d, const double *X_dev, const double *y_dev, const pmh_svm_opts *opts, pmh_svm *svm);
/* The training samples stored in float32 (pmh_op_create_svm_dual_f32): X_dev is n_local x d floats.  alpha, w, b, the solvers and the model stay fp64 and every
   other entry (set_labels, set_penalties, set_subset, train, predict_own, test_own, ...) works unchanged on the handle.  d != 64: a training gives bit for bit
   what pmh_svm_create gives on the widened samples */
int pmh_svm_create_f32(pmh_ctx ctx, int n_local, int d, const float *X_dev, const double *y_dev, const pmh_svm_opts *opts, pmh_svm *svm);
int pmh_svm_train(pmh_svm svm);                                     /* from a = 0: MPGP (no bias) or SMALXE + MPGP (bias), then the model */
/* Warm starts: a training from the handle's last dual instead of zero -- along a path of penalties C_1 < C_2 < ..., or from one subset (fold) to the next.
 * The handle keeps alpha and a flag "alpha is the dual of a training with the current labels": pmh_svm_train and pmh_svm_train_warm set it,
 * pmh_svm_set_labels clears it, pmh_svm_set_penalties and pmh_svm_set_subset leave alpha and the flag as they are (a promise).  Only one GPU is tested; under a
 * communicator the start vector is elementwise and local and the multiplier's scalar is the same on every rank.
 * pmh_svm_warm_start_vector: a0_i = m_i ? min(max(alpha_scale alpha_i, 0), ub_i) : 0 in exactly this order of operations, one kernel launch; m the current
 * subset mask (all ones without one), ub_i the current upper bound (L1: C_i; L2: none).  It leaves two counts on the handle (pmh_svm_get_warm_start_counts,
 * summed over the ranks): entries the mask zeroed that were not zero, and entries clipped at ub.  alpha_scale not positive and finite: PMH_ERR_ARG; no dual of
 * the current labels (never trained, or pmh_svm_set_labels since): PMH_ERR_STATE.
 * pmh_svm_train_warm: pmh_svm_train, except that alpha starts as that vector (formed by the same function, in place) and, with a bias, SMALXE starts from the
 * last training's multiplier (pmh_smalxe_set_initial_multiplier): B'mu_0 = (b_prev sqrt(n_S)) row, b_prev the last pmh_svm_stats::b_multiplier, row and n_S the
 * current ones -- so it survives a new subset.  Statistics, passes_X, the model and the clearing of the calibration as in pmh_svm_train; a refusal changes
 * nothing.  pmh_svm_train itself is untouched by any of this: after a warm training it gives what a fresh handle gives, bit for bit */
int pmh_svm_warm_start_vector(pmh_svm svm, double alpha_scale, double *a0_dev /* n_local doubles */);
int pmh_svm_get_warm_start_counts(pmh_svm svm, long long *masked /* or NULL */, long long *clipped /* or NULL */); /* of the last start vector formed (0, 0 before any) */
int pmh_svm_train_warm(pmh_svm svm, double alpha_scale);
int pmh_svm_get_model(pmh_svm svm, double *w_host /* d doubles, or NULL */, double *b /* or NULL */);
int pmh_svm_get_dual(pmh_svm svm, double *alpha_dev);               /* n_local doubles */
int pmh_svm_get_stats(pmh_svm svm, pmh_svm_stats *st);
int pmh_svm_get_solver(pmh_svm svm, pmh_op *H, pmh_qppf *pf, pmh_mpgp *mpgp, pmh_smalxe *smalxe); /* borrowed; any pointer may be NULL, a solver not in use comes back NULL */
/* A penalty per sample, C_i = (y_i > 0 ? C_pos : C_neg) weight_i, in place of the one C of the options (unbalanced classes; weighted samples):
 *   L1: 0 <= a_i <= C_i;   L2: 0 <= a_i, Hessian H + diag(1 / C_i) (pmh_op_svm_dual_set_diag on the handle's operator, in place of the scalar 1/C).
 * Free support vectors (the bias) are counted against C_i.  Call it after create, and again between trainings at will (pmh_svm_train starts from a = 0; the last dual stays on the handle for pmh_svm_train_warm); the
 * handle is untrained afterwards and its solver is built anew, so handles from pmh_svm_get_solver must be fetched again.  weight_dev: n_local doubles on the
 * device, copied, or NULL = all 1.  C_pos / C_neg not positive and finite: PMH_ERR_ARG naming the value.  Weights that are not positive and finite (zero
 * included: a weight does not leave a sample out, pmh_svm_set_subset does): PMH_ERR_ARG saying how many, counted on the device, over all ranks.  Nothing is exchanged in training
 * that was not before: the bounds and the diagonal are local vectors */
int pmh_svm_set_penalties(pmh_svm svm, double C_pos, double C_neg, const double *weight_dev /* n_local doubles or NULL = all 1; copied */);
/* the effective C_i (n_local doubles, device); opts.C everywhere if pmh_svm_set_penalties was never called */
int pmh_svm_get_penalties(pmh_svm svm, double *c_dev /* n_local */);
/* New labels on the created handle, X staying where it is (no upload, no new column-ordered copy; pmh_op_svm_dual_set_labels).  y_dev: n_local doubles of +-1,
 * borrowed in place of the old ones; it may be the buffer lent at creation with new contents.  The equality's row y / sqrt(n) is refilled and its one-row
 * projector rebuilt (bias); the penalties go back to the scalar opts.C (L1: ub = C; L2: the diagonal comes off, the shift is 1 / C; pmh_svm_get_penalties
 * answers C everywhere) -- set them again afterwards: labels, then penalties; the handle is untrained and its solver built anew (handles from
 * pmh_svm_get_solver must be fetched again).  A training afterwards gives alpha, w, b and every counter of the statistics identical to those of a fresh handle
 * created on (X, y_dev) with the same options.  Allowed under a communicator: nothing is collective beyond what create does */
int pmh_svm_set_labels(pmh_svm svm, const double *y_dev /* n_local doubles, borrowed */);
/* Train on a subset S of the handle's samples and score the held-out rows, X staying where it is (no upload, no new column-ordered copy).  m_dev as in
 * pmh_op_svm_dual_set_subset (copied; NULL: all samples again).  Over S only: the operator's subset, rhs = m, the equality's row m o y / sqrt(n_S) (n_S summed
 * over the ranks as n is), L2 the diagonal m_i / C_i in place of the shift; L1 keeps its bounds C_i.  The solver is built anew (as by pmh_svm_set_penalties),
 * the handle is untrained and uncalibrated afterwards; a refused mask (PMH_ERR_ARG) leaves the handle as it was.  pmh_svm_set_labels and pmh_svm_set_penalties
 * keep the subset.  After pmh_svm_train alpha is exactly 0 on the held-out rows and w, b, n_sv, n_free_sv are those of training on (X[S], y[S]) alone */
int pmh_svm_set_subset(pmh_svm svm, const double *m_dev /* n_local doubles of 0 / 1, or NULL = all */);
/* the mask (n_local doubles, device; all 1 without a subset; may be NULL) and n_S over all ranks (n without a subset; may be NULL) */
int pmh_svm_get_subset(pmh_svm svm, double *m_dev, long long *n_in);
/* Scores and labels of ALL n_local samples the handle was created on, held-out ones included, by the sweep of pmh_svm_predict(_csr) over the handle's own X
   (CSR: with the tables the operator holds): the same bits as pmh_svm_predict on an uploaded copy.  Either pointer may be NULL */
int pmh_svm_predict_own(pmh_svm svm, double *scores_dev, double *labels_dev);
/* (TP, FP, TN, FN) of the handle's own samples against its labels, over the rows `which` selects, in one sweep (fixed order, no float atomics).
   PMH_SVM_OWN_HELD_OUT without a subset: PMH_ERR_STATE; PMH_SVM_OWN_SUBSET without a subset: all rows */
#define PMH_SVM_OWN_HELD_OUT 0
#define PMH_SVM_OWN_SUBSET 1
#define PMH_SVM_OWN_ALL 2
int pmh_svm_test_own(pmh_svm svm, int which, long long counts[4]);
/* one pass over the n samples of X_dev: scores_dev[i] = x_i . w + b, labels_dev[i] = +-1 (either may be NULL) */
int pmh_svm_predict(pmh_svm svm, int n, const double *X_dev, double *scores_dev, double *labels_dev);
/* one pass: counts = (TP, FP, TN, FN) of the predicted labels against y_dev (summed over the ranks under a communicator) */
int pmh_svm_test(pmh_svm svm, int n, const double *X_dev, const double *y_dev, long long counts[4]);
/* Test samples in float32 (n x d floats), for any handle with d <= 256 whatever it was trained on -- fp64, float32 or CSR samples; a handle created on float32
   samples likewise scores fp64 and CSR test samples through the entries above and below.  Same limits and messages as the fp64 entries */
int pmh_svm_predict_f32(pmh_svm svm, int n, const float *X_dev, double *scores_dev, double *labels_dev);
int pmh_svm_test_f32(pmh_svm svm, int n, const float *X_dev, const double *y_dev, long long counts[4]);
/* Samples in CSR (any d; see pmh_op_create_svm_dual_csr): X and y_dev borrowed.  Every other entry works unchanged on the handle.  Test samples may come in
   either form whatever the training samples were: pmh_svm_predict / pmh_svm_test need d <= 256, the _csr entries a matrix of the model's d columns; a
   mismatch is PMH_ERR_ARG */
int pmh_svm_create_csr(pmh_ctx ctx, pmh_csr X, const double *y_dev, const pmh_svm_opts *opts, pmh_svm *svm);
int pmh_svm_predict_csr(pmh_svm svm, pmh_csr Xt, double *scores_dev, double *labels_dev);
int pmh_svm_test_csr(pmh_svm svm, pmh_csr Xt, const double *y_dev, long long counts[4]);
int pmh_svm_destroy(pmh_svm svm);

/* ---- SVM with more than two classes: one-vs-rest (svm_multi.hip) --------------------------------------------------------------------------------------------
 * The classes are the distinct values of the n labels, ascending: c_0 < .. < c_{K-1}, K >= 2.  Training solves the K binary problems "class k (+1) against the
 * rest (-1)" one after the other on ONE binary handle over X (pmh_svm_set_labels between them: X is uploaded once, the CSR operator's column-ordered copy is
 * built once) and keeps W (K x d, row k = the w of class k) and b (K).  K = 2 trains two classifiers; pmh_svm is there for that case.  balanced: class k is
 * trained with C_pos = C n / (2 n_k), C_neg = C n / (2 (n - n_k)) (pmh_svm_set_penalties, no sample weights), n_k the samples of class k; else C for both.
 * Prediction is ONE pass over the test samples for up to pmh_svm_multi_chunk classes (per kernel path), ceil(K / chunk) passes in all: scores S[i,k] = x_i . W_k + b_k (n x K,
 * row-major) and labels[i] = c_k of the greatest score of row i; ties go to the lowest class index; NaN scores are not a case.  No float atomics and a fixed
 * summation order: two calls give the same bits, and scores-only, labels-only and both give the same arrays.  One GPU: a context with a communicator on is
 * PMH_ERR_ARG, as are a label that is not finite and fewer than two classes.  X and labels_dev are borrowed. */
typedef struct pmh_svm_multi_s *pmh_svm_multi;
int pmh_svm_multi_chunk(int path, int *KC); /* classes per pass over the test samples, a compile-time constant per kernel path: 0 dense d = 64, 1 dense any d, 2 CSR */
int pmh_svm_multi_create(pmh_ctx ctx, int n, int d, const double *X_dev, const double *labels_dev, const pmh_svm_opts *opts, int balanced, pmh_svm_multi *svm);
int pmh_svm_multi_create_csr(pmh_ctx ctx, pmh_csr X, const double *labels_dev, const pmh_svm_opts *opts, int balanced, pmh_svm_multi *svm);
int pmh_svm_multi_train(pmh_svm_multi svm);
int pmh_svm_multi_get_classes(pmh_svm_multi svm, int *K, double *classes_host /* K, ascending; NULL to ask K */);
/* the model; before pmh_svm_multi_train / pmh_svm_multi_set_model: PMH_ERR_STATE */
int pmh_svm_multi_get_model(pmh_svm_multi svm, double *W_host /* K x d row-major, or NULL */, double *b_host /* K, or NULL */);
/* a saved model: the handle counts as trained afterwards (it has no statistics) */
int pmh_svm_multi_set_model(pmh_svm_multi svm, const double *W_host, const double *b_host);
/* the statistics of class k's training (st may be NULL; PMH_ERR_STATE before pmh_svm_multi_train) and the penalties it is trained with (either may be NULL) */
int pmh_svm_multi_get_stats(pmh_svm_multi svm, int k, pmh_svm_stats *st, double *C_pos, double *C_neg);
/* scores_dev: n x K, labels_dev: n, either may be NULL.  Dense test samples need d <= 256, CSR test samples the model's d columns, whichever form the training
   samples had; a mismatch is PMH_ERR_ARG.  Before a model exists: PMH_ERR_STATE */
int pmh_svm_multi_predict(pmh_svm_multi svm, int n, const double *X_dev, double *scores_dev, double *labels_dev);
int pmh_svm_multi_predict_csr(pmh_svm_multi svm, pmh_csr Xt, double *scores_dev, double *labels_dev);
/* confusion[t K + p] = the samples of true class c_t predicted as c_p (K x K, host; integer atomics: counts have no order); a true label that is no class
   is counted in *n_unknown (may be NULL) and in no cell */
int pmh_svm_multi_test(pmh_svm_multi svm, int n, const double *X_dev, const double *labels_true_dev, long long *confusion, long long *n_unknown);
int pmh_svm_multi_test_csr(pmh_svm_multi svm, pmh_csr Xt, const double *labels_true_dev, long long *confusion, long long *n_unknown);
/* Train the K problems on a subset S of the handle's samples, X staying where it is (pmh_svm_set_subset of the one binary handle, which pmh_svm_set_labels and
 * pmh_svm_set_penalties between the classes keep).  m_dev as in pmh_svm_set_subset (copied; NULL: all samples again).  The classes stay those of ALL training
 * labels: K, the classes, the shape of W and the chunks do not change.  A class without a sample in S is PMH_ERR_ARG, the message giving the class value (its
 * problem against the rest would have no positive sample); what pmh_svm_set_subset refuses (an entry that is neither 0 nor 1, an empty S) is passed on.  A
 * refusal leaves the handle as it was: subset, model, statistics, calibration.  On success the handle is untrained (pmh_svm_multi_get_model: PMH_ERR_STATE),
 * without statistics and uncalibrated; pmh_svm_multi_set_model keeps the subset.  balanced under a subset: C_pos = C n_S / (2 n_{k,S}), C_neg = C n_S /
 * (2 (n_S - n_{k,S})), the counts over S (pmh_svm_multi_get_stats reports them) */
int pmh_svm_multi_set_subset(pmh_svm_multi svm, const double *m_dev /* n doubles of 0 / 1, or NULL = all samples; copied */);
/* the mask (n doubles, device; all 1 without a subset), n_S (n without a subset) and the samples of each class inside S (K, host); each may be NULL */
int pmh_svm_multi_get_subset(pmh_svm_multi svm, double *m_dev /* n, or NULL */, long long *n_in /* or NULL */, long long *class_counts_host /* K, or NULL */);
/* Scores (n x K) and labels (n) of ALL n samples the handle was created on, held-out ones included, nothing uploaded: the sweeps of pmh_svm_multi_predict(_csr)
   over the handle's own X (CSR: its own pmh_csr), the same bits as on an uploaded copy.  Either pointer may be NULL.  Before a model exists: PMH_ERR_STATE */
int pmh_svm_multi_predict_own(pmh_svm_multi svm, double *scores_dev /* n x K, or NULL */, double *labels_dev /* n, or NULL */);
/* confusion (K x K, host, as pmh_svm_multi_test's) of the handle's own samples against its training labels over the rows `which` selects; *n_counted (may be
   NULL): how many rows that is.  Dense samples: a row that is not selected is not loaded from X; CSR: every stored entry is swept (no row skipping, as on the
   binary handle) and only the count selects.  PMH_SVM_OWN_HELD_OUT without a subset: PMH_ERR_STATE; PMH_SVM_OWN_SUBSET without a subset: all rows; any other
   `which`: PMH_ERR_ARG */
int pmh_svm_multi_test_own(pmh_svm_multi svm, int which /* PMH_SVM_OWN_HELD_OUT | _SUBSET | _ALL */, long long *confusion /* K x K */, long long *n_counted /* or NULL */);
int pmh_svm_multi_destroy(pmh_svm_multi svm);

/* ---- SVM probabilities: Platt scaling (svm_proba.hip) --------------------------------------------------------------------------------------------------------
 * P(y = +1 | x) = 1 / (1 + exp(A s(x) + B)), s the score x . w + b.  A, B minimise the regularised negative log-likelihood
 *   F(A, B) = - sum_i (t_i log p_i + (1 - t_i) log(1 - p_i)),  t_i = (n_pos + 1) / (n_pos + 2) for y_i = +1, 1 / (n_neg + 2) for y_i = -1,
 * by Newton's method with backtracking: the algorithm of H.-T. Lin, C.-J. Lin, R. C. Weng, "A note on Platt's probabilistic outputs for support vector
 * machines", Machine Learning 68 (2007), with its constants (LIBSVM's sigmoid_train).  Every evaluated point (A, B) is ONE launch over the n scores that
 * gives F, the gradient and the Hessian (six sums, fixed order, no float atomics: two fits give the same bits); six doubles cross to the host per point.
 * Under a communicator the scores are sharded as the samples are and the sums and class counts are all-reduced.
 * pmh_svm_platt_fit: n < 1 (over all ranks) or a label that is not +-1: PMH_ERR_ARG (the message says how many).  One class only: the start point A = 0,
 * B = log((n_neg + 1) / (n_pos + 1)) is stationary and is returned.  Separable scores: A runs off until the iteration limit or the line search ends the fit;
 * the last accepted (finite) point is returned, reason says which.  The caller supplies the calibration samples (held-out ones, or the training set). */
enum { PMH_PLATT_CONVERGED = 1, PMH_PLATT_MAX_IT = 2, PMH_PLATT_LINE_SEARCH = 3 };
typedef struct {
  int       reason;                  /* PMH_PLATT_CONVERGED | _MAX_IT | _LINE_SEARCH (0: the calibration was set, not fitted) */
  int       iterations, evaluations; /* Newton steps taken; launches of the sums kernel */
  long long n_pos, n_neg;
  double    fval, g1, g2;            /* F and its gradient at the returned point */
} pmh_svm_platt_stats;
int pmh_svm_platt_fit(pmh_ctx ctx, int n, const double *scores_dev, const double *y_dev, double *A, double *B, pmh_svm_platt_stats *st /* or NULL */);
/* The binary handle: calibrate scores the samples as pmh_svm_predict(_csr) does and fits A, B on those scores (the result is pmh_svm_platt_fit of
 * pmh_svm_predict's scores, bit for bit); set_calibration takes a saved pair.  A calibration belongs to a model: pmh_svm_train, pmh_svm_set_labels and
 * pmh_svm_set_penalties clear it.  predict_proba: proba_dev[i] = 1 / (1 + exp(A (x_i . w + b) + B)) in ONE pass over the samples, the dot product summed as
 * pmh_svm_predict sums it.  Untrained handle (calibrate), no calibration (predict_proba, get_calibration): PMH_ERR_STATE */
int pmh_svm_calibrate(pmh_svm svm, int n, const double *X_dev, const double *y_dev);
int pmh_svm_calibrate_f32(pmh_svm svm, int n, const float *X_dev, const double *y_dev); /* the calibration samples in float32 (pmh_svm_predict_f32's scores) */
int pmh_svm_calibrate_csr(pmh_svm svm, pmh_csr Xt, const double *y_dev);
int pmh_svm_set_calibration(pmh_svm svm, double A, double B);
int pmh_svm_get_calibration(pmh_svm svm, double *A, double *B, pmh_svm_platt_stats *st /* or NULL */);
int pmh_svm_predict_proba(pmh_svm svm, int n, const double *X_dev, double *proba_dev);
int pmh_svm_predict_proba_f32(pmh_svm svm, int n, const float *X_dev, double *proba_dev); /* the samples in float32 */
int pmh_svm_predict_proba_csr(pmh_svm svm, pmh_csr Xt, double *proba_dev);
/* One-vs-rest: one scoring call (pmh_svm_multi_predict's), then K fits, fit k on column k of the scores with "label == c_k" as +1 and every other label (a
 * value that is no class included) as -1.  predict_proba (n x K): sigma_ik = 1 / (1 + exp(A_k S[i,k] + B_k)) written by the scoring sweeps, then every row
 * divided by its sum (k ascending); a row sum of 0 gives 1 / K everywhere.  pmh_svm_multi_train and pmh_svm_multi_set_model clear the calibration;
 * pmh_svm_multi_predict stays the arg-max of the raw scores */
int pmh_svm_multi_calibrate(pmh_svm_multi svm, int n, const double *X_dev, const double *labels_dev);
int pmh_svm_multi_calibrate_csr(pmh_svm_multi svm, pmh_csr Xt, const double *labels_dev);
int pmh_svm_multi_set_calibration(pmh_svm_multi svm, const double *A_host /* K */, const double *B_host /* K */);
int pmh_svm_multi_get_calibration(pmh_svm_multi svm, double *A_host /* K, or NULL */, double *B_host /* K, or NULL */, pmh_svm_platt_stats *st_host /* K, or NULL */);
int pmh_svm_multi_predict_proba(pmh_svm_multi svm, int n, const double *X_dev, double *proba_dev);
int pmh_svm_multi_predict_proba_csr(pmh_svm_multi svm, pmh_csr Xt, double *proba_dev);

/* ---- SVR: linear epsilon-insensitive support vector regression (svr_train.hip) --------------------------------------------------------------------------------
 * Samples X (n x d), targets t (all finite), epsilon >= 0, C > 0, optional sample weights: C_i = C weight_i.
 *   L1: primal 1/2 |w|^2 + sum C_i max(0, |x_i . w + b - t_i| - eps);    L2: primal 1/2 |w|^2 + 1/2 sum C_i max(0, |x_i . w + b - t_i| - eps)^2
 *   dual in u = [p; q] (2 n doubles):  min 1/2 u'H^u - c^'u,  H^ the operator of pmh_op_create_svr_dual with D = 0 (L1) or diag(1 / C_i) (L2),
 *   c^ = [t - eps; -t - eps];  L1: 0 <= u <= [C_i; C_i];  L2: 0 <= u;  bias: additionally sum (p_i - q_i) = 0, posed as the unit row [1; -1] / sqrt(2 n).
 * Without bias the QP goes to MPGP, with bias to SMALXE over pmh_qppf_create_onerow, the penalty absorbed by the operator as its rank-one term -- the route of
 * pmh_svm_train.  Model: w = X'(p - q), f(x) = x . w + b.  b_free is the mean over the free entries of the box (astol < u_k and, L1, u_k < C_i - astol; astol
 * the inner MPGP's) of  t_i - eps - D_i p_i - x_i . w  (a free p_i)  and  t_i + eps + D_i q_i - x_i . w  (a free q_i): stationarity in a free entry.
 * b_multiplier = mu / sqrt(2 n), mu the multiplier of the row in the Lagrangian 1/2 u'H^u - c^'u + mu (row'u).  The bias returned is b_free, or b_multiplier
 * where no entry is free; without bias it is 0.  The bias and the counts take one pass over X, in a fixed summation order.
 * Not here: warm starts, a grid search.  Sharding by rows under a communicator is kept in the code, one GPU is tested. */
typedef struct {
  int             loss_type;  /* -svr_loss_type L1 | L2 (PMH_SVM_LOSS_L1 | PMH_SVM_LOSS_L2) */
  double          C;          /* -svr_C, > 0 */
  double          epsilon;    /* -svr_epsilon, >= 0 */
  int             bias;       /* -svr_bias 0 | 1 */
  pmh_qps_opts    qps;        /* as in pmh_svm_opts */
  pmh_mpgp_opts   mpgp;
  pmh_smalxe_opts smalxe;
} pmh_svr_opts;
typedef struct {
  int       reason;                             /* converged reason of the training solve */
  int       outer_iterations, inner_iterations; /* as in pmh_svm_stats */
  int       nmv, ncg, nexp, nprop;
  long long passes_X;                           /* passes over X of the solve */
  long long n_sv, n_free_sv;                    /* entries of [p; q] above astol, free ones */
  double    sum_beta;                           /* sum (p_i - q_i) of the returned dual */
  double    b, b_free, b_multiplier;            /* the bias returned, the mean over the free entries (NaN: none), the multiplier's value */
  double    rho, normBu, rnorm;                 /* as in pmh_svm_stats */
} pmh_svr_stats;
typedef struct {
  long long n, n_in_tube;                       /* samples; those with |r_i| <= eps, r_i = f(x_i) - t_i */
  double    sum_r, sum_r2, sum_abs_r, max_abs, sum_t, sum_t2; /* the sums of the one pass, each in a fixed order */
  double    mse, mae, r2;                       /* sum_r2 / n, sum_abs_r / n, 1 - sum_r2 / (sum_t2 - sum_t^2 / n) (NaN for n == 0; r2 NaN for constant targets) */
} pmh_svr_metrics;
typedef struct pmh_svr_s *pmh_svr;
int pmh_svr_default_opts(pmh_svr_opts *o); /* L1, C = 1, epsilon = 0.1, bias */
/* -svr_loss_type, -svr_C, -svr_epsilon, -svr_bias here; everything else through pmh_qps_set_from_options with the empty prefix */
int pmh_svr_set_from_options(const char *options, pmh_svr_opts *o, char *unknown, int unknown_cap);
/* X_dev, t_dev (n_local doubles) borrowed.  epsilon < 0 or not finite, C <= 0, a target that is not finite (counted on the device): PMH_ERR_ARG with the value */
int pmh_svr_create(pmh_ctx ctx, int n_local, int d, const double *X_dev, const double *t_dev, const pmh_svr_opts *opts, pmh_svr *svr);
int pmh_svr_create_f32(pmh_ctx ctx, int n_local, int d, const float *X_dev, const double *t_dev, const pmh_svr_opts *opts, pmh_svr *svr);
int pmh_svr_create_csr(pmh_ctx ctx, pmh_csr X, const double *t_dev, const pmh_svr_opts *opts, pmh_svr *svr);
/* C_i = C weight_i (weight_dev: n_local doubles, copied; NULL: all 1) with the checks and messages of pmh_svm_set_penalties; the solver is built anew and the
   handle is untrained afterwards */
int pmh_svr_set_penalties(pmh_svr svr, double C, const double *weight_dev);
/* A new epsilon: the right-hand side alone changes, the handle is untrained afterwards.  MPGP (no bias) is kept; SMALXE sizes eta by |c^| when it is created,
   so with a bias the solver is built anew (the operator, its CSR copy and the projector stay).  Either way a training afterwards gives a fresh handle's bits */
int pmh_svr_set_epsilon(pmh_svr svr, double epsilon);
int pmh_svr_train(pmh_svr svr); /* from u = 0 */
int pmh_svr_get_model(pmh_svr svr, double *w_host /* d doubles, or NULL */, double *b /* or NULL */); /* before training: PMH_ERR_STATE */
int pmh_svr_get_dual(pmh_svr svr, double *u_dev /* 2 n_local doubles: p, then q */);
int pmh_svr_get_stats(pmh_svr svr, pmh_svr_stats *st);
int pmh_svr_get_solver(pmh_svr svr, pmh_op *H, pmh_qppf *pf, pmh_mpgp *mpgp, pmh_smalxe *smalxe); /* borrowed, as pmh_svm_get_solver */
/* f(x_i) = x_i . w + b in one pass over the test samples.  Dense test samples need d <= 256, CSR ones the model's d columns, whatever the handle was trained on */
int pmh_svr_predict(pmh_svr svr, int n, const double *X_dev, double *f_dev);
int pmh_svr_predict_f32(pmh_svr svr, int n, const float *X_dev, double *f_dev);
int pmh_svr_predict_csr(pmh_svr svr, pmh_csr Xt, double *f_dev);
/* scores and reduces in the same pass: the sums of pmh_svr_metrics (the tube is the handle's epsilon), turned into mse, mae, r2 on the host */
int pmh_svr_test(pmh_svr svr, int n, const double *X_dev, const double *t_dev, pmh_svr_metrics *m);
int pmh_svr_test_f32(pmh_svr svr, int n, const float *X_dev, const double *t_dev, pmh_svr_metrics *m);
int pmh_svr_test_csr(pmh_svr svr, pmh_csr Xt, const double *t_dev, pmh_svr_metrics *m);
/* Train on a subset S of the handle's samples and score the held-out rows, X staying where it is (no upload, no new column-ordered copy).  m_dev as in
 * pmh_op_svr_dual_set_subset (copied; NULL: all samples again, and a training then has the bits of a handle that never had a subset).  Over S only: the
 * operator's subset, c^_S = [m o (t - eps); m o (-t - eps)], the equality's row [m; -m] / sqrt(2 n_S) (n_S summed over the ranks), L2 the D term; L1 keeps its
 * bounds.  The solver is built anew and the handle is untrained afterwards; a refused mask leaves the handle exactly as it was.  pmh_svr_set_epsilon and
 * pmh_svr_set_penalties keep the subset.  After pmh_svr_train u is exactly 0 on the held-out rows in both halves and w, b, n_sv, n_free_sv, sum_beta are those
 * of training on (X[S], t[S]) alone */
int pmh_svr_set_subset(pmh_svr svr, const double *m_dev /* n_local doubles of 0 / 1, or NULL = all */);
/* the mask (n_local doubles, device; all 1 without a subset; may be NULL) and n_S over all ranks (n without a subset; may be NULL) */
int pmh_svr_get_subset(pmh_svr svr, double *m_dev, long long *n_in);
/* f(x_i) for all samples the handle was created on, held-out ones included, nothing uploaded: bit for bit pmh_svr_predict on the same X (CSR: the row sweep with
   the operator's own tables) */
int pmh_svr_predict_own(pmh_svr svr, double *f_dev /* n_local doubles */);
/* pmh_svr_test over the handle's own samples and targets: which = PMH_SVM_OWN_HELD_OUT | PMH_SVM_OWN_SUBSET | PMH_SVM_OWN_ALL selects the rows the seven sums
   and the metrics are taken over (m->n: the selected rows over all ranks; every row is still swept).  PMH_SVM_OWN_HELD_OUT without a subset: PMH_ERR_STATE;
   PMH_SVM_OWN_SUBSET without a subset: all rows */
int pmh_svr_test_own(pmh_svr svr, int which, pmh_svr_metrics *m);
int pmh_svr_destroy(pmh_svr svr);

/* ---- random Fourier features: Z[i, k] = scale cos(sum_j X[i, j] omega[j, k] + beta[k]) (rff.hip) ------------------------------------------------
 * With the columns of omega drawn from a shift-invariant kernel's spectral density, beta uniform on [0, 2 pi) and scale = sqrt(2 / D), z(x) . z(x') ~ k(x, x'):
 * pmh_svm_create / pmh_svm_multi_create / pmh_svr_create on Z (n x D row-major, D <= 256) train an approximate kernel machine, and the scoring entries take the
 * map of the test samples.  The caller draws omega and beta: the library holds no random generator.  One kernel on the fp64 matrix cores; all arithmetic fp64
 * whatever the storage types; every row is summed in an order fixed by d alone, without atomics: a sample has the same features alone and in any batch. */
typedef struct pmh_rff_s *pmh_rff;
enum { PMH_F64 = 0, PMH_F32 = 1 }; /* the type an array is stored in */
/* omega_dev: d x D row-major, copied; beta_dev: D doubles, copied (NULL: all 0).  d < 1, D < 1, a scale that is not finite, an entry of omega or beta that is not
 * finite (counted on the device): PMH_ERR_ARG with a message */
int pmh_rff_create(pmh_ctx ctx, int d, int D, const double *omega_dev, const double *beta_dev, double scale, pmh_rff *f);
/* X_dev: n x d row-major doubles (PMH_F64) or floats (PMH_F32: a value enters as (double)x); Z_dev: n x D row-major doubles or floats (rounded once, at the store).
 * n = 0 launches nothing.  Another type code, n < 0: PMH_ERR_ARG.  Enqueues on the context's stream */
int pmh_rff_apply(pmh_rff f, long long n, const void *X_dev, int x_type, void *Z_dev, int z_type);
/* any pointer may be NULL; omega_host: d D doubles, beta_host: D doubles */
int pmh_rff_get(pmh_rff f, int *d, int *D, double *omega_host, double *beta_host, double *scale);
/* info = {rows per workgroup, rows per wave, column tile, k-block, LDS bytes, waves per workgroup, classes per chunk of pmh_rffdots, LDS bytes of its kernel} */
int pmh_rff_info(pmh_rff f, int info[8]);
/* tests: the same kernel with the identity in place of scale cos(.): T_dev (n x D doubles) = X omega + beta */
int pmh_rff_test_args(pmh_rff f, long long n, const void *X_dev, int x_type, double *T_dev);
int pmh_rff_destroy(pmh_rff f);

/* ---- scoring on the features without storing them (rff_score.hip) ---------------------------------------------------------------------------------------
 * dots_dev[i K + k] = sum_c scale cos(x_i . omega_c + beta_c) W_dev[k ldw + c], c < D: the dot products of the features of X (as pmh_rff_apply reads it) with the K
 * rows of a model W (K x D row-major doubles, row stride ldw >= D); no bias is added and no n x D array exists.  The classes go through the map's kernel in
 * chunks of info[6]; a chunk's features are computed anew (K = 10: three times).  Each product enters its sum by a fused multiply-add; a sum's order is fixed
 * by d and D alone, without atomics: a sample's dots have the same bits alone and in any batch, and a class's dots whatever K is and wherever the class sits.
 * n = 0 launches nothing.  n < 0, K < 1, ldw < D, another type code, a NULL pointer with n > 0: PMH_ERR_ARG.  D > 256: n ceil(D / 256) info[6] doubles of
 * workspace for the length of the call */
int pmh_rffdots(pmh_rff f, long long n, const void *X_dev, int x_type, int K, const double *W_dev, int ldw, double *dots_dev);
/* tests: the same kernel with the identity in place of scale cos(.): dots_dev = (X omega + beta) W' */
int pmh_rffdots_test_args(pmh_rff f, long long n, const void *X_dev, int x_type, int K, const double *W_dev, int ldw, double *dots_dev);
/* The scoring entries of the three front ends on MAPPED samples: (map, n, X_dev, x_type) stands where the dense entries take (n, X_dev) -- X_dev: n x map.d
 * row-major of x_type -- and the handle scores the features map(X) it would be given by pmh_rff_apply, through pmh_rffdots against its model and then through
 * the kernels that finish its CSR paths (n K doubles of workspace for the call); everything after the samples is the dense entry's.  map.D must be the handle's
 * d: PMH_ERR_ARG naming both.  The state checks (trained, calibrated) are the dense entries'.  The handle's sample type does not matter: the features are fp64
 * and never rounded, so a handle trained on float32 features scores features here that were not rounded to float32 */
int pmh_svm_predict_rff(pmh_svm svm, pmh_rff map, int n, const void *X_dev, int x_type, double *scores_dev, double *labels_dev);
int pmh_svm_test_rff(pmh_svm svm, pmh_rff map, int n, const void *X_dev, int x_type, const double *y_dev, long long counts[4]);
int pmh_svm_calibrate_rff(pmh_svm svm, pmh_rff map, int n, const void *X_dev, int x_type, const double *y_dev);
int pmh_svm_predict_proba_rff(pmh_svm svm, pmh_rff map, int n, const void *X_dev, int x_type, double *proba_dev);
int pmh_svm_multi_predict_rff(pmh_svm_multi svm, pmh_rff map, int n, const void *X_dev, int x_type, double *scores_dev, double *labels_dev);
int pmh_svm_multi_test_rff(pmh_svm_multi svm, pmh_rff map, int n, const void *X_dev, int x_type, const double *labels_true_dev, long long *confusion, long long *n_unknown);
int pmh_svm_multi_calibrate_rff(pmh_svm_multi svm, pmh_rff map, int n, const void *X_dev, int x_type, const double *labels_dev);
int pmh_svm_multi_predict_proba_rff(pmh_svm_multi svm, pmh_rff map, int n, const void *X_dev, int x_type, double *proba_dev);
int pmh_svr_predict_rff(pmh_svr svr, pmh_rff map, int n, const void *X_dev, int x_type, double *f_dev);
int pmh_svr_test_rff(pmh_svr svr, pmh_rff map, int n, const void *X_dev, int x_type, const double *t_dev, pmh_svr_metrics *m);

/* ---- Nystroem features: Z = k(X, L) M (nys.hip) -----------------------------------------------------------------------------------------------------------
 * L: m landmarks taken from the data; M (m x D) = U_r Lambda_r^{-1/2} from k(L, L) = U Lambda U', so that z(x) . z(x') = k(x, L) k(L, L)^+ k(L, x') ~ k(x, x').
 *   PMH_NYS_RBF   k(x, l) = exp(-gamma |x - l|^2), |x - l|^2 = max((|x|^2 + |l|^2) - 2 x . l, 0)      PMH_NYS_POLY  k(x, l) = (gamma x . l + coef0)^degree
 * The caller chooses the landmarks and computes M: the library holds no random generator and no eigen-solver.  Z is what pmh_svm_create / pmh_svm_multi_create /
 * pmh_svr_create take.  Two kernels on the fp64 matrix cores per chunk of rows (C = k(X, L) into a workspace of chunk rows x m doubles, then Z = C M); all
 * arithmetic fp64 whatever the storage types; no atomics; every sum in an order fixed by d and m alone: a sample has the same features alone and in any batch,
 * whatever the chunk size.  |x - l|^2 comes from norms and a product: for a sample that is itself a landmark it is of the order of u d |x|^2, not exactly 0. */
typedef struct pmh_nys_s *pmh_nys;
enum { PMH_NYS_RBF = 0, PMH_NYS_POLY = 1 };
/* landmarks_dev: m x d row-major, copied; M_dev: m x D row-major, copied.  d, m or D < 1, D > m, another kernel code, a gamma that is not positive and finite, a
 * coef0 that is not finite, a degree outside 1 .. 16 (all three are checked for either kernel), an entry of the landmarks or of M that is not finite (counted on
 * the device): PMH_ERR_ARG with a message */
int pmh_nys_create(pmh_ctx ctx, int d, int m, int D, const double *landmarks_dev, int kernel, double gamma, double coef0, int degree, const double *M_dev, pmh_nys *f);
/* C_dev (n x m row-major doubles) = k(X, L), with no workspace.  X_dev: n x d row-major doubles (PMH_F64) or floats (PMH_F32: a value enters as (double)x).
 * n = 0 launches nothing.  Another type code, n < 0: PMH_ERR_ARG.  Enqueues on the context's stream */
int pmh_nys_kernel(pmh_nys f, long long n, const void *X_dev, int x_type, double *C_dev);
/* Z_dev (n x D row-major doubles or floats: rounded once, at the store) = k(X, L) M, chunk by chunk; otherwise as pmh_nys_kernel */
int pmh_nys_apply(pmh_nys f, long long n, const void *X_dev, int x_type, void *Z_dev, int z_type);
/* any pointer may be NULL; landmarks_host: m d doubles, M_host: m D doubles */
int pmh_nys_get(pmh_nys f, int *d, int *m, int *D, int *kernel, double *gamma, double *coef0, int *degree, double *landmarks_host, double *M_host);
/* info = {rows per workgroup, rows per wave, column tile, k-block, LDS bytes of the kernel behind pmh_nys_kernel, waves per workgroup, chunk rows, workspace bytes
 * (INT_MAX if they are more)} */
int pmh_nys_info(pmh_nys f, int info[8]);
/* the rows of C that exist at a time in pmh_nys_apply: a positive multiple of info[0], else PMH_ERR_ARG; the workspace is allocated anew.  No result depends on it */
int pmh_nys_set_chunk_rows(pmh_nys f, long long rows);
/* tests: the kernel behind pmh_nys_kernel with an identity in place of the kernel function: T_dev (n x m doubles) = X L' (what = 0), or the |x - l|^2 the rbf map
 * exponentiates (what = 1; on a PMH_NYS_POLY map: PMH_ERR_ARG) */
int pmh_nys_test_args(pmh_nys f, long long n, const void *X_dev, int x_type, int what, double *T_dev);
int pmh_nys_destroy(pmh_nys f);


/* ---- PC for the inner KSP of MATINV: multigrid V-cycle (PCMG semantics) ----------------------------------------
 * The reference's iterative MATINV applies K^+ with a PETSc KSP whose PC is chosen by -mat_inv_pc_type
 * (src/mat/impls/inv/matinv.c, MatInvGetKSP / MatInvSetUp).  pmh_mg is that PC on the device for PCMG-like set-ups:
 * A[0] is the fine operator (the same CSR the MATBLOCKDIAG holds), A[l+1] = P[l]' A[l] P[l] are handed over by the
 * caller, P[l] is n_l x n_{l+1}.  Smoother: Chebyshev of the given degree on D^-1 A over
 * [lo_frac, hi_frac] x lambda_max[l] (PETSc's PCMG/GAMG default is 0.1, 1.1), applied before and after the coarse
 * correction; the coarsest level is solved block-wise by the dense (pseudo-)inverses in coarse_pinv (row-major blocks
 * of sizes coarse_rowstart[b+1]-coarse_rowstart[b], concatenated).  The CSR handles stay owned by the caller.
 * precision: PMH_MG_FP64, or PMH_MG_FP32 = the cycle (operators, vectors, coarse inverses) in single precision -- it only
 * preconditions the fp64 CG; needs 3x3-block operators (elasticity, PETSc's BAIJ bs=3 case) on every smoothed level. */
#define PMH_MG_FP64 0
#define PMH_MG_FP32 1
#define PMH_MG_FP16 2 /* as FP32, the fine-level operator stored as (scaled) fp16 entries */
typedef struct pmh_mg_s *pmh_mg;
int pmh_mg_create(pmh_ctx ctx, int nlevels, const pmh_csr *A, const pmh_csr *P, int degree, const double *lambda_max, double lo_frac, double hi_frac, int nb_coarse, const int *coarse_rowstart,
                  const double *coarse_pinv_host, int precision, pmh_mg *mg);
/* The same PC with the hierarchy built HERE (host C++, runs once) for a block-diagonal A_fine whose blocks are Q1 discretisations on
 * boxes of dims[3 b .. 3 b + 2] nodes (x fastest, node-major dofs, ndof per node): trilinear prolongations (x) I_ndof (exact for rigid-body
 * modes), Galerkin operators, lambda_max(D^-1 A) by the power method, dense pseudo-inverses of the coarsest blocks
 * (A + Q Q')^{-1} - Q Q' with Q the kernel basis injected from R_host (kdim x n, zero over non-singular blocks; NULL if none floats).
 * Coarsening stops at <= min_nodes nodes per block; congruent blocks are processed once.  rowptr / col / val: host copy of A_fine. */
int pmh_mg_create_box(pmh_ctx ctx, pmh_csr A_fine, int nblocks, const int *block_rowstart, const int *dims, int ndof, const int *rowptr, const int *col, const double *val, int kdim,
                      const double *R_host, int min_nodes, int degree, int precision, pmh_mg *mg);
/* The same PC with an ALGEBRAIC hierarchy built HERE (host C++, runs once) for blocks of ANY shape -- subdomains that are not boxes, what a mesh partitioner hands
 * the reference, whose MATINV factorises any block (src/mat/impls/inv/matinv.c:481-580) and whose iterative path takes -mat_inv_pc_type gamg: smoothed aggregation
 * (Vanek, Mandel, Brezina 1996).  Per level: node graph (ndof dofs per node on the fine level, one node per aggregate below), couplings kept where the Frobenius norm
 * of their block exceeds theta * 0.5^level * sqrt(|A_ii| |A_jj|), greedy aggregates, a tentative prolongation that reproduces the block's near-kernel exactly, one
 * damped-Jacobi smoothing step of it, Galerkin operators; coarsening stops when every block has <= max_coarse dofs (every block is coarsened equally often);
 * congruent blocks are processed once.  Near-kernel of a block: its kernel vectors where R_host (kdim x n) is non-zero over it (a floating block: the rigid-body
 * modes; such a block stays consistently singular down the hierarchy and its coarsest operator gets a pseudo-inverse), else the rows of nns_host (nns x n; NULL or
 * zero over the block: the ndof translations).  A near-kernel of 3 or 6 vectors keeps 3 x 3 blocks on every level (PMH_MG_FP32 / PMH_MG_FP16 and the
 * multi-right-hand-side solver apply).  rowptr / col / val: host copy of A_fine. */
int pmh_mg_create_sa(pmh_ctx ctx, pmh_csr A_fine, int nblocks, const int *block_rowstart, int ndof, const int *rowptr, const int *col, const double *val, int kdim, const double *R_host,
                     int nns, const double *nns_host, int max_coarse, double theta, int degree, int precision, pmh_mg *mg);
/* host routine (tests, diagnostics): the aggregates pmh_mg_create_sa forms on ONE level of one block -- A: n x n host CSR with bs dofs per node; agg_out[n / bs] */
int pmh_sa_aggregate(int n, int bs, const int *rowptr, const int *col, const double *val, double theta, int *agg_out, int *n_agg);
/* host routine (tests, sanitizer runs; no device): the whole hierarchy pmh_mg_create_sa builds for ONE block (R: kdim x n kernel vectors; kdim = 0: a non-singular block, near-kernel = the
   ndof translations).  level_rows[0 .. *nlevels): rows per level (room for 16); defect[0] = max_l max|A_l B_l| / max|A_l|, defect[1] = max_l max|P_l B_{l+1} - B_l| (both 0 for kdim = 0),
   defect[2] = max|A_c A_c^+ A_c - A_c| / max|A_c| of the coarsest operator and its dense (pseudo-)inverse */
int pmh_sa_hierarchy_host(int n, int ndof, const int *rowptr, const int *col, const double *val, int kdim, const double *R, int max_coarse, double theta, int *nlevels, int *level_rows, double *defect);
int pmh_mg_apply(pmh_mg mg, const double *b_dev, double *x_dev); /* x = V(b), zero initial guess (PCApply) */
int pmh_mg_stats(pmh_mg mg, long long *fine_spmv);
int pmh_mg_timing_enable(pmh_mg mg, int max_launches); /* HIP-event pairs around the fine-level operator launches */
int pmh_mg_timing_get(pmh_mg mg, int *launches, double *total_ms, double *bytes_per_launch);
int pmh_mg_destroy(pmh_mg mg);
/* Test entries (tests/test_gpu_mg_paths.py): the V-cycle as an operator, one column (pmh_mg) and 8 interleaved columns (the multi-right-hand-side form inside K^+).
 * pmh_mg_test_info: info = {rows of the level, level operator (0 CSR / none on the coarsest level, 1 blocks of 3 x 3), its storage (PMH_BSR_*, -1 without a block copy),
 *   transfer kernels to the next level (0 none, 1 node-wise, 2 scalar short rows, 3 scalar long rows), the level runs fused, cycle precision (0 fp64, 1 fp32), coarse
 *   pseudo-inverse in fp16, every coarse block a multiple of 16 rows and >= 512, coarse blocks, congruent replicas of the block copy}; cp_scale: the fp16 pseudo-inverse's
 *   power of two.
 * pmh_mg_test_apply: pmh_mg_apply under a device halt word of the entry's own holding `halt` (non-zero: every launch must be a no-op); synchronises.
 * pmh_mg_test_vector: one work vector of a level to the host in the cycle's precision -- which = 0 x, 1 b, 2 r, 3 d, 4 t, 5 xa, 6 dinv; PMH_ERR_ARG for a vector the
 *   level does not own (x, b of level 0 in fp64; all but x, b on the coarsest level).
 * pmh_mg_mv_test_create: the 8-column cycle on the hierarchy of mg (of the first of nrep congruent blocks); PMH_ERR_SUP with the reason where it declines.
 * pmh_mg_mv_test_info: info = {rows per replica, nrep, transfer kernels (0 none, 1 node-wise, 2 rectangular ELL pair, 3 scalar), coarse solve on the last level (0 fp32
 *   entries, 1 fp16 entries, 2 fp16 on the matrix cores; -1 on a smoothed level), storage of the level operator's copy (-1 on the last level), the next level's first
 *   direction rides on the restriction, coarse blocks per replica, 0}.
 * pmh_mg_mv_test_apply: b (and z64, or NULL as the solver calls it) fp64 device multivectors of rows x 8; pmh_mg_mv_test_vector: as above in float, rows x 8 (dinv: rows). */
int pmh_mg_test_info(pmh_mg mg, int level, long long info[10], double *cp_scale);
int pmh_mg_test_apply(pmh_mg mg, const double *b_dev, double *x_dev, int halt);
int pmh_mg_test_vector(pmh_mg mg, int level, int which, void *host_out);
int pmh_mg_mv_test_create(pmh_mg mg, int nrep, void **M);
int pmh_mg_mv_test_info(void *M, int level, long long info[8]);
int pmh_mg_mv_test_apply(void *M, const double *b_dev, double *z64_dev, int halt);
int pmh_mg_mv_test_vector(void *M, int level, int which, float *host_out);
int pmh_mg_mv_test_destroy(void *M);
int pmh_matinv_set_pc_mg(pmh_matinv Kplus, pmh_mg mg); /* NULL: back to Jacobi / none */
/* MATINV's own K x product on the 3x3-block kernel (PETSc MATSEQBAIJ role: 8.44 instead of 12 bytes per non-zero);
 * returns PMH_ERR_SUP if K has no 3x3 block structure.  Timing as pmh_csr_timing_*. */
int pmh_matinv_enable_bsr3(pmh_matinv Kplus);
int pmh_matinv_bsr3_replicas(pmh_matinv Kplus, int *nrep); /* congruent blocks sharing the one device copy of the 3x3-block operator (1: a copy per block / no such copy) */
int pmh_matinv_timing_enable(pmh_matinv Kplus, int max_launches);
int pmh_matinv_timing_get(pmh_matinv Kplus, int *launches, double *total_ms, double *bytes_per_launch);

/* ---- QPS PCPG (src/qps/impls/pcpg/pcpg.c:51-134) -------------------------------------------------------- */
typedef struct {
  int    iteration, reason;
  double rnorm;
} pmh_pcpg_stats;
/* pc: NULL (none) or an operator applied as z = M^{-1} w (PCApply), e.g. the lumped dual preconditioner */
int pmh_pcpg_solve(pmh_ctx ctx, pmh_op A, const double *b, double *x, pmh_qppf pf, pmh_op pc, double rtol, double atol, double divtol, int max_it, pmh_pcpg_stats *st);

/* ---- QPS KSP (src/qps/impls/ksp/qpsksp.c:127-143): the solver QPSSetDefaultType picks for a QP without box or
 * equality constraints (qps.c:437-449), e.g. the projected dual of a linear TFETI problem or the FETI-1 dual.
 * The KSP is the one QPSCreate_KSP sets up (qpsksp.c:244-250): CG, unpreconditioned residual norm, x as initial
 * guess, pc NULL = PCNONE; stopping test QPSKSPConverged_KSP -> QPSConvergedDefault. */
int pmh_ksp_cg_solve(pmh_ctx ctx, pmh_op A, const double *b, double *x, pmh_op pc, double rtol, double atol, double divtol, int max_it, pmh_pcpg_stats *st);

/* ---- KSPFETI (src/ksp/impls/feti/feti.c): KSPFETISetUp (:71-94) + KSPSolve_FETI (:144-156) for a decomposed linear problem ----
 * Input = what the reference holds after QPTMatISToBlockDiag (qptransform.c:2007-2150): the block-diagonal K (host CSR, blocks
 * given by block_rowstart), f split among the copies of shared dofs, l2g (global dof of every local dof), the Dirichlet dofs to be
 * enforced by B (local indices, KSPFETISetDirichlet(..., FETI_LOCAL, PETSC_TRUE); none if they are eliminated in K), and the
 * kernel vectors R (kdim rows of length N, zero over non-floating blocks; orthonormalised internally).
 * Builds B = [B_d; B_g] (QPFetiAssembleDirichlet, QPFetiGetBgtSF), K^+ (MatRegularize + MATINV, or the Moore-Penrose wrapping),
 * G = R'B', the dual QP chain, solves it with the QPS the reference's QPSSetDefaultType picks (CG on P F, optional lumped / Dirichlet PC) and
 * recovers u.  One call per solve; everything it creates is released before it returns. */
typedef struct {
  int    gluing_type;        /* -feti_gluing_type: 0 nonred, 1 full (default, qpfeti.c:322), 2 orth */
  int    scale;              /* -SCALE_ON (default 1) */
  int    exclude_dirichlet;  /* -feti_gluing_exclude_dirichlet (default 0) */
  int    regularize;         /* -regularize (default 1, qptransform.c:2215); 0: -qpt_dualize_Kplus_mp */
  int    kplus_left;         /* -qpt_dualize_Kplus_left (DEFAULT 1): K^+ = K^- P_R with the fixing dofs of MatRegularize as null pivots (pmh_matinv_set_left_inverse).  The reference switches to it,
                                and to -regularize 0, by itself whenever the QP came without a kernel and it computed one (qptransform.c:997-1008) -- always the case under KSPFETI, which
                                never sets one (feti.c:71-94; feti/ex1.c, ex71.c).  0: `regularize` decides (K_reg^{-1} or the Moore-Penrose form).  Ignored with explicit_dual (K^- P_R is not symmetric) */
  int    project;            /* -project (default 1, set by -feti: QPTEnforceEqByProjector).  0: the equality constraint G lambda = e stays in the dual QP, which is homogenised and
                                handed to QPS SMALXE (QPSSetDefaultType qps.c:437-441; QPTEnforceEqByPenalty inside SMALXE) -- `smalxe` below configures it */
  int    E_orth_type;        /* -dual_qp_E_orth_type (QPTOrthonormalizeEqFromOptions qptransform.c:643-660; MatOrthTypes): 0 none, 1 gs / 2 gslingen (explicit T G, T e), 3 cholesky / 4 implicit (G stays sparse, the projector carries T = L^{-1}) */
  int    lumped_pc;          /* -dual_pc_dual_type (PCDualTypes, default none): 0 none, 1 lumped (B K B'), 2 dirichlet (B S B', pmh_op_create_pc_dual_dirichlet) */
  double regularize_rho;     /* > 0: the rho of MatRegularize for every block; 0 (default): the reference's power-method estimate */
  double kplus_rtol; int kplus_max_it; /* inner KSP of MATINV */
  double rtol, atol, divtol; int max_it; /* -qps_rtol ... of the dual solve (qps.c:73-76) */
  int    max_it_set;         /* 1: max_it was given (-qps_max_it, or by the caller): with project == 0 it replaces QPSCreate_SMALXE's own default of 100 (smalxe.c:1203) whatever its value */
  int    explicit_dual; double explicit_rtol; /* 1: F applies through the explicit local dual operators (pmh_fexplicit_*), assembled at explicit_rtol (default 0 / 1e-13) */
  /* the reference's post-solve report, QPChainPostSolve (src/qp/interface/qpchain.c:198-275): */
  int    view_convergence;   /* -qps_view_convergence: "  last QPSSolve CONVERGED due to ..., KSPReason=.., required .. iterations" (qps.c:1188-1230) */
  int    view_kkt;           /* -qp_chain_view_kkt: the `r = ...` lines of QPViewKKT (qp.c:245-369) for EVERY QP of the chain, last to first: projected dual, homogenised dual, dual
                                (twice: QPTScale always adds a child sharing all vectors, qptransform.c:1459), decomposed primal (twice), assembled original */
  int    matis_to_diag_norm; /* -qpt_matis_to_diag_norm: the "Dirichlet in Hess: .., r = ||Ax-b|| = .." line of QPTPostSolve_QPTMatISToBlockDiag (qptransform.c:1954-1979), and its
                                side effect on the two QPs printed after it when the Dirichlet dofs are enforced by B (see pmh_kspfeti_solve in kspfeti.hip) */
  char  *view_buf; int view_cap; /* the text (full PETSc viewer lines, '\n'-separated, NUL-terminated, truncated to view_cap) goes here; NULL: to stdout */
  pmh_smalxe_opts smalxe;    /* -qps_smalxe_* / -qps_smalxe_qps_* of the SMALXE solve taken with project == 0 (its outer tolerances are rtol / atol / divtol / max_it above) */
  int    kplus_pc;           /* -dual_mat_inv_pc_type: 0 jacobi (default: what the golden tests pin), 1 gamg = the algebraic V-cycle built inside the library (pmh_mg_create_sa) on the
                                matrix MATINV inverts, near-kernel = the kernel vectors R -- subdomains of any shape, any of the three generalised inverses */
  int    kplus_pc_ndof;      /* dofs per node of the aggregation's node graph; 0: 3 where the blocks come with 6 kernel vectors and 3 | their sizes, else 1 */
} pmh_kspfeti_opts;
typedef struct {
  int    iteration, reason;  /* CG iterations on P F; with project == 0 SMALXE's outer iterations */
  double rnorm;              /* ||P (F lambda - d)|| at exit; with project == 0 SMALXE's max(||G x||, ||g||) */
  int    n_lambda, n_dirichlet_rows, coarse_dim;
  pmh_smalxe_stats smalxe;   /* filled with project == 0 */
} pmh_kspfeti_stats;
/* vector part of QPTMatISToBlockDiag (qptransform.c:2095-2113: assembled rhs -> copies, interface values divided by their
   multiplicity) and of its post-solve (:1945-1949: INSERT_VALUES assembly of the solution, no averaging); host routines */
int pmh_qpt_matis_split_rhs(int N, const int *l2g, int n_global, const double *b_global, double *f_local);
int pmh_qpt_matis_assemble_solution(int N, const int *l2g, const double *u_local, int n_global, double *x_global);
/* matrix side of QPTMatISToBlockDiag (qptransform.c:2007-2150): MATIS = per-subdomain local matrices + l2g  ->  the MATBLOCKDIAG of the child QP
   (MatCreateBlockDiag(comm, matis->A)) in the concatenated local numbering, matis->counter (dof multiplicities: D = 1/counter), the interface
   flags of the local dofs and i2g = the sorted global interface dofs (QPFetiSetInterfaceToGlobalMapping); host routine.  loc_rowptr: the
   subdomains' row pointers one after the other (n_s + 1 entries each, each starting at 0); col / val / counter / is_interface / i2g may be NULL */
int pmh_qpt_matis_to_blockdiag(int nsub, const int *l2g_start, const int *l2g, int n_global, const int *loc_rowptr, const int *loc_col, const double *loc_val, int *block_rowstart,
                               int *rowptr, int *col, double *val, int *counter, int *is_interface, int *n_i2g, int *i2g);
int pmh_kspfeti_default_opts(pmh_kspfeti_opts *o);
/* the options-database keys of the FETI chain (-feti_gluing_type, -feti_gluing_exclude_dirichlet, -SCALE_ON, -regularize,
   -qpt_dualize_Kplus_mp, -dual_pc_dual_type, -qps_rtol/-qps_atol/-qps_divtol/-qps_max_it, -dual_mat_inv_ksp_rtol/_max_it, -dual_mat_inv_pc_type jacobi | gamg) */
int pmh_kspfeti_set_from_options(const char *options, pmh_kspfeti_opts *o, char *unknown, int unknown_cap);
int pmh_kspfeti_solve(pmh_ctx ctx, int nsub, const int *block_rowstart, const int *rowptr, const int *col, const double *val, const double *f, const int *l2g, int n_dir,
                      const int *dir_local, int kdim, const double *R, const pmh_kspfeti_opts *o, double *u_host, double *lambda_host /* or NULL */, int lambda_cap,
                      pmh_kspfeti_stats *st);

/* ---- TFETI contact problem in one call (QPTFromOptions / QPTAllInOne, src/qp/interface/qptransform.c:2152-2237: dualize ->
 * orthonormalize -> homogenize -> project; QPSSetDefaultType -> SMALXE + MPGP; the post-solve chain) ----------------------------------
 * Input = the decomposed QP: block-diagonal K (host CSR), f, the constraint matrix B as leaves (local primal dof, dual row, value) with
 * the n_eq equality rows (gluing, Dirichlet) first and the inequality rows (B_I u <= c_I, e.g. non-penetration) after them, c, the
 * kernel vectors R (kdim x N; every block floats in TFETI), optionally the blocks' node boxes (dims: nsub x 3, x fastest, node-major
 * dofs) for the multigrid PC of K^+.  K^+ = P_R K^- P_R (-regularize 0 -qpt_dualize_Kplus_mp); with explicit_dual the explicit local dual
 * operators carry F (exact, one dense SYMV per apply).  Output: u (N, host), lambda (n_lambda, host, optional), the solver's statistics. */
typedef struct {
  pmh_smalxe_opts smalxe;           /* outer tolerances + SMALXE / inner MPGP parameters (pmh_smalxe_default_opts) */
  double kplus_rtol; int kplus_max_it;
  int    mg, mg_min_nodes, mg_degree, mg_precision; /* multigrid PC of the inner KSP: the box hierarchy when dims != NULL (pmh_mg_create_box), else the algebraic one
                                                       (pmh_mg_create_sa on the kernel vectors; max_coarse = 3 mg_min_nodes): blocks of any shape */
  int    bsr3;                      /* K x of the inner CG on the 3x3-block kernel when ndof == 3 */
  int    explicit_dual; double explicit_rtol; int explicit_storage; /* explicit_dual: 0 / positive / PMH_KPLUS_AUTO, see below; storage: pmh_fexplicit_* (PMH_FX_SYM / PMH_FX_FULL / PMH_FX_CLASS /
                                                                 PMH_FX_CLASS_SYM / PMH_FX_CLASS_ORBIT) */
  int    orthonormalize;            /* QPTOrthonormalizeEq: 1 G <- L^{-1} G formed explicitly, 2 implicitly (G stays sparse, -qp_E_orth_form implicit), 0 none */
  int    explicit_symmetry;         /* PMH_FX_CLASS_SYM / _ORBIT with dims != NULL: the symmetries of the box (pmh_fexplicit_set_box_symmetry) serve the set-up / the storage */
  double expected_applies;          /* explicit_dual == PMH_KPLUS_AUTO: the F applications the caller expects the solve to take; 0: PMH_KPLUS_AUTO_DEFAULT_APPLIES */
} pmh_feti_contact_opts;
/* explicit_dual: 0 the inner Krylov K^+ in every F application; any positive value (default 1) the explicit local dual operators; PMH_KPLUS_AUTO the choice between the two
 * by the estimated time to solution.  The probe (after the hierarchy, the gluing and the projector exist): one timed F application through the inner Krylov K^+ on a fixed
 * pseudo-random lambda (after one untimed one), t_it; the explicit storage planned exactly as explicit_dual = 1 plans it and the first batch of its set-up solves run and
 * timed, t_batch (the batch is kept if the explicit path is chosen); the dense apply estimated from the planned storage, t_ex = bytes / 5.87 TB/s (k_fx_symv, whole F
 * application, storage PMH_FX_SYM on the 43^3-scale staircase cut) or, PMH_FX_CLASS_ORBIT, useful flops / 36.5 TFLOP/s (k_fxo_gemm16 on configs[2]).  Explicit iff
 *   n_batches t_batch + A t_ex < A t_it,   n_batches = the set-up batches still to run, A = expected_applies (0: PMH_KPLUS_AUTO_DEFAULT_APPLIES);
 * then exactly the path of explicit_dual = 1 or 0 runs.  F applications of one default solve (rtol 1e-5), measured: configs[2] (2 x 2 x 2 boxes of 43^3 elements, orbit
 * storage) 196, the staircase cut of feti.irregular_partition at 21^3 scale 165 and at 43^3 scale 207 (profiles/r07_kplus_auto_staircase43.txt); the default A = 250 is the
 * largest of them with some room.  With it the rule picks explicit on configs[2] and the inner Krylov K^+ on both staircase cuts. */
#define PMH_KPLUS_AUTO (-1)
#define PMH_KPLUS_AUTO_DEFAULT_APPLIES 250
typedef struct {
  pmh_smalxe_stats smalxe;
  int    n_lambda, n_eq, coarse_dim, n_active, explicit_solves;
  double setup_seconds, solve_seconds, explicit_seconds, norm_Glambda_minus_e;
  int    explicit_symmetries;       /* operations used by the set-up by symmetry (0 / 1: none) */
  int    kplus_path;                /* the K^+ of F this solve ran: 0 inner Krylov, 1 explicit local dual operators (every call) */
  int    kplus_auto;                /* 1: explicit_dual == PMH_KPLUS_AUTO chose it */
  long long setup_solves_planned;   /* K^+ solves of the explicit set-up as planned (the explicit path and the probe; the self-check of the set-up by symmetry included) */
  double expected_applies_used, est_explicit_seconds, est_iterative_seconds; /* PMH_KPLUS_AUTO: A and the two sides of the rule */
  double probe_seconds;             /* PMH_KPLUS_AUTO: wall time of the probe (inside setup_seconds; its set-up batch is reused when the explicit path is chosen) */
  int    f_applies;                 /* F applications of the SMALXE solve (set-up and post-solve not counted) */
} pmh_feti_contact_stats;
int pmh_feti_contact_default_opts(pmh_feti_contact_opts *o);
int pmh_feti_contact_solve(pmh_ctx ctx, int nsub, const int *block_rowstart, const int *rowptr, const int *col, const double *val, const double *f, int n_lambda, int n_eq, int n_leaves,
                           const int *leaves_row, const int *leaves_root, const double *leaves_val, const double *c, int kdim, const double *R, const int *dims /* or NULL */, int ndof,
                           const pmh_feti_contact_opts *o, double *u_host, double *lambda_host /* or NULL */, pmh_feti_contact_stats *st);

/* ---- bench-only shims (csrc/bench_shims.hip: written over the public hooks above, nothing inside the solvers) --------------------------------
 * pmh_mpgp_run_fixed: exactly `iters` MPGP iterations (rtol = atol = 0, max_it = iters - 1 around pmh_mpgp_solve; the test is evaluated every iteration);
 * pmh_smalxe_run_fixed: the real SMALXE loop for exactly `inner_iters` inner iterations in total (inner iteration limit = what is left of the budget; a solve
 * that converges earlier restarts from u = 0 after pmh_smalxe_reset; counts accumulate over the restarts). */
int pmh_mpgp_run_fixed(pmh_mpgp s, int iters);
int pmh_smalxe_run_fixed(pmh_smalxe s, int inner_iters, int *solves, int *outer_iters, int *ncg, int *nexp, int *nprop, int *nmv);

/* ---- multi-right-hand-side K^+ (csrc/mv.hip, mg_mv.hip, matinv_mv.hip): PMH_MV_R = 8 columns per block solved together on interleaved multivectors
 * V[(dof) * 8 + column] -- the column-blocked set-up of the explicit inverse (MatInvExplicitly_Inv, src/mat/impls/inv/matinv.c:640-730: MatMatSolve on blocks of
 * right-hand sides) for blocks with NO symmetry and NO congruence: every 3 x 3 block of K_b is loaded once for the 8 columns.
 * pmh_mv_test_spmv: the operator product alone (measurement / test entry): Y = A X for a resident CSR of 3 x 3 blocks and 8 columns, entries kept in `storage`
 * (0 fp64, 1 fp32, 2 fp16 with fp32 vectors); x, y: device, 8 n doubles; the average launch time of `repeats` products through HIP events. */
int pmh_mv_test_spmv(pmh_csr A, int storage, const double *x, double *y, int repeats, float *ms_per_launch);
/* ---- multi-right-hand-side product test entries (csrc/mv.hip: the ELL builders as the V-cycle and the block CG call them, and one launch of k_mv_spmv; nothing inside the
 * solvers changes) ----
 * pmh_mv_test_create: the ELL copy of the CSR A with entries kept in `storage` (0 fp64, 1 fp32, 2 fp16 scaled by a power of two, fp32 arithmetic).  kind 0: square, the
 * FIRST of nrep congruent diagonal blocks (PMH_ERR_ARG where that block's rows do not end at nnz / nrep or reach beyond its own columns); 1: rectangular; 2: rectangular,
 * the copy holds -A (nrep = 1 for both).  *E = NULL with PMH_SUCCESS where the builder declines: no rows, 3 not dividing rows or columns, kind 0 and not square, 3 nrep
 * not dividing the rows or nrep the entries, a row with unsorted or repeated columns, no block at all or a block row of more than 2048, a padded copy beyond 2 GB.
 * pmh_mv_test_info: info = {block rows, block columns, W = slots per block row, lanes per block row (4 / 16), storage, workgroups per launch, XCD order of the workgroups
 * (0 / 1), kind}; *scale (or NULL): the fp16 scale (1 otherwise), negative for a negated fp16 copy (whose stored entries are those of A).
 * pmh_mv_test_mult_epi: one launch with the epilogue `epi` on device multivectors of 8 columns -- double for fp64 storage, float otherwise (z64: always double); x:
 * 3 (block columns) 8 entries, y, y1, r, d, z64: 3 (block rows) 8, dinv: 3 (block rows), one per ROW:
 *   0 NONE y = A x;  1 ADD y = y1 + A x (y1 may be y);  2 SUB y = A x - y1;  10 PRE y = c0 x + c2 dinv (y1 - A x);  11 POST1 r = dinv (y1 - A x), d = c0 r, y = x + d;
 *   12 POST2 y += c1 x + c2 (r - dinv A x), z64 (or NULL) = (double)y;  20 RESTRICT y = A x and, d != NULL, d = (dinv c0) y.
 * halt != 0: the launch sees a device flag set to 1 and changes nothing.  Synchronises.  PMH_ERR_ARG, and no launch, for an unknown epilogue, an operand the epilogue
 * needs and does not get, an output that is x, and 10 / 11 / 12 on a rectangular copy (they read x at the row's own offset). */
int pmh_mv_test_create(pmh_csr A, int storage, int kind, int nrep, void **E);
int pmh_mv_test_info(void *E, long long info[8], double *scale);
int pmh_mv_test_mult_epi(void *E, int epi, const void *x, void *y, const void *y1, const void *dinv, void *r, void *d, double *z64, double c0, double c1, double c2, int halt);
int pmh_mv_test_destroy(void *E);
/* ---- CSR product test entries (csrc/spmv.hip: read the plan, or wrap one launch; nothing inside the solvers changes) ----------------------------------------
 * pmh_csr_kernel_info: the kernel plan pmh_csr_create chose for A.  info[0]: path of a plain product -- 0 ELL (slot-major copy), 1 stream with one lane per row,
 * 2 medium stream with 8 lanes per row, 3 vector, 4 long-row chunks; info[1]: ELL width or lanes per row (1, 8, 32, 64), 0 for long-row chunks; info[2]: 1 when the
 * plain product reads 16-bit column offsets; info[3]: entries per row block (paths 1, 2) or the number of chunks (path 4), else 0; info[4]: row blocks (ELL:
 * blocks of 256 rows); info[5]: partial slots the MPGP epilogue finalises (0 without rows).  With the MPGP epilogue, long-row matrices run the stream kernel of
 * path 1 (info[4] row blocks).  *uid (or NULL): the matrix's unique, non-zero identity.
 * pmh_csr_test_mult_epi: one product y = A x with the epilogue `kind` -- 0 none, 1 ADD (y = y1 + A x, y1 may be y), 2 SUB (y = A x - y1), 3 MPGP (y = A x, A square;
 * scal_host = p'Ap, g'p and the feasible step QPCFeas(xx, p) of p = x, lb / ub may be NULL).  halt != 0: the launch sees a device flag set to 1 and changes
 * nothing.  Device vectors; synchronises. */
int pmh_csr_kernel_info(pmh_csr A, int info[6], unsigned long long *uid);
int pmh_csr_test_mult_epi(pmh_csr A, int kind, const double *x, const double *y1, const double *g, const double *xx, const double *lb, const double *ub, int halt, double *y,
                          double scal_host[3]);
/* ---- test entries of the dual-space chain behind a penalised operator (csrc/qppf.hip, csrc/dualchain.hip; nothing inside the solvers changes) -----------------------
 * pmh_op_penalized_test_mult_epi: one application to the device vector x.  kind 0: y = A_rho x.  kind 2: the gradient split of MPGP -- y = g = A_rho x - b, gf, p = gf
 * (device vectors; lb may be NULL), the block partials of (0, |gP|^2, |gc|^2, |gf|^2) -> partials_host[4][*nblocks] and the segment sums of G0 p the last kernel emitted
 * -> psums_host[*nseg] (both at most cap doubles per row).  same_input != 0: the caller asserts that x still holds what the operator was last applied to.  Synchronises.
 * PMH_ERR_SUP where the operator does not run on the chain.
 * pmh_op_penalized_test_emit: what 0: the caller is about to change x or p without emission (pmh_op_s::emit_invalidate); what 1: a kernel that writes the iterate x and
 * leaves the segment sums of G0 x behind (here: x as it is). */
int pmh_op_penalized_test_mult_epi(pmh_op op, int kind, int same_input, const double *x, const double *b, const double *lb, double astol, double *y, double *gf, double *p, int cap,
                                   double *partials_host, double *psums_host, int *nblocks, int *nseg);
int pmh_op_penalized_test_emit(pmh_op op, int what, const double *x);
/* ---- test entries of the MPGP phase kernels and the reduction finishers (csrc/mpgp.hip, csrc/vec.hip, csrc/emit_inline.h; nothing inside the solvers changes) ------
 * They overwrite the context's block partials and scalar slots, which every solve writes before it reads them.  All of them synchronise.
 * pmh_vec_test_finalize: ONE launch of k_finalize on K <= 8 caller-chosen rows (rows_host[K][nblocks], nblocks <= 2048), quantity k reduced with ops[k] (0 SUM, 1 MIN)
 * into scalar slot slots[k] (0..63).  scal_dev / scal_pinned [K]: in, what the device slot / its pinned mirror hold before the launch; out, what they hold afterwards.
 * halt < 0: no halt word, else a device word of that value.  post_inc (or NULL): the two device counters the launch bumps, in / out.
 * pmh_mpgp_test_host_sum_row: the host's own last step of a reduction (host_sum_row of mpgp.hip) on row[nb], nb <= 512, op 0 SUM / 1 MIN.
 * pmh_mpgp_test_block_sum: pmh_sum_block_partials of row_host[nb] (nb <= 512) in one wave; out_host[64] = what every lane returns.
 * pmh_mpgp_test_block_partials: pmh_block_partials<3> with (SUM, SUM, MIN) in workgroups of 1024 threads, thread t of workgroup b holding entry 1024 b + t of the
 * device vectors a, b, c (past the end: 0, 0, +inf); dev_host / pinned_host [3][nblocks]: in, what the device rows / the pinned rows hold before; out, afterwards.
 * pmh_mpgp_test_phase: ONE launch of the phase kernel `phase` on the caller's device vectors (see the struct), as solve_fused / solve_unfused launch it.
 * pmh_mpgp_test_set_gradient_valid: the carried gradient as SMALXE hands it over (fused driver only): g (device, n doubles) is copied into the solver's gradient vector
 * and the NEXT pmh_mpgp_solve takes it as A x - b at its starting point instead of forming it.
 * pmh_mpgp_test_spec_words: after a solve, words[0] = 1 where the solver set up the speculative device-side CG chain (only where it may use it), words[1..4] = halt,
 * iteration, ncg, base as the last batch left them. */
typedef struct {
  double       *x, *g, *p, *Ap, *gf;  /* device vectors of n entries; a phase touches those its kernel takes (phase 6: gP = x, gc = g) */
  const double *lb, *ub, *b;          /* device; lb / ub may be NULL; b: phase 7 */
  pmh_op        op;                   /* emit: NULL, the emission targets are off; else a penalised operator on the dual-space chain, asked for them through emit_begin as the driver asks */
  double       *partials_dev, *partials_pinned; /* HOST [8][2048]: in, the block partials on the device / in the pinned copy before the launch; out, afterwards */
  double        astol, afeas, alpha, acg_host, pAp_host;
  double        ttol, divtol_rhs, gamma2;       /* SPEC: the constants of pmh_spec_args */
  double        ring[48];                       /* SPEC: the monitor ring, in / out */
  double        scal_dev[64], scal_pinned[64];  /* in, every scalar slot on the device / in the pinned mirror before the launch; out, afterwards */
  int           emit;     /* 1: the 1024-thread variant */
  int           spec;     /* phase 1: the device-side verdict (needs use_ctl, setp = 0, emit = 0) */
  int           setp;     /* phase 1: the proportioning form (p = gf) */
  int           finalize; /* 1: followed by the driver's finalising launch of that phase (phases 0, 1, 5, 6, 7) */
  int           use_ctl;  /* 1: the control words go to the device; phases 1 (SPEC), 2 and the finalising launch run under ctl[0] and bump ctl[1], ctl[2] */
  int           nb;       /* emit: block partials to add -- phase 1 (rows 4, 5: acg; 0: acg_host), phase 2 (row 0) */
  int           ring_cap, max_it;
  int           ctl[4];   /* halt, iteration, ncg, base: in / out */
} pmh_mpgp_phase_test;
enum { PMH_PHASE_SPLIT = 0, PMH_PHASE_STEP, PMH_PHASE_DIR, PMH_PHASE_PROP_DIR, PMH_PHASE_EXPANSION, PMH_PHASE_P1_DOTS, PMH_PHASE_THREE_NORMS, PMH_PHASE_OBJ };
int pmh_vec_test_finalize(pmh_ctx ctx, int K, int nblocks, const double *rows_host, const int *ops, const int *slots, int halt, int *post_inc, double *scal_dev, double *scal_pinned);
int pmh_mpgp_test_host_sum_row(const double *row, int nb, int op, double *out);
int pmh_mpgp_test_block_sum(pmh_ctx ctx, int nb, const double *row_host, double *out_host);
int pmh_mpgp_test_block_partials(pmh_ctx ctx, int n, const double *a, const double *b, const double *c, double *dev_host, double *pinned_host);
int pmh_mpgp_test_phase(pmh_ctx ctx, int phase, int n, pmh_mpgp_phase_test *t);
int pmh_mpgp_test_set_gradient_valid(pmh_mpgp s, const double *g);
int pmh_mpgp_test_spec_words(pmh_mpgp s, int words[5]);
/* ---- further test entries of the dual-space chain (csrc/dualchain.hip, csrc/qppf.hip) -----------------------------------------------------------------------------
 * pmh_op_test_create_staged: F = scatter middle gather from three device CSR matrices (gather nmid x n, middle nmid x nmid, scatter n x nmid) as an operator that
 * answers pmh_op_s::stages, its middle stage pmh_csr_mult; its plain product is the three products.  Under pmh_op_create_penalized(pmh_op_create_projected(F, pf, 1),
 * pf, rho) with an implicitly orthonormalised pf it runs on the chain.  Destroyed by pmh_op_destroy; the matrices stay the caller's.
 * pmh_op_penalized_test_chain_info: info = {n, m, tiles, segments, W (8 / 16), NU (2 / 8), listed gather rows, records with a partner row, gather rows with more than
 * 3 entries, scatter rows with more than 2 entries}.  PMH_ERR_SUP where the operator does not run on the chain.
 * pmh_op_penalized_test_chain_read: what 0..2 the segment sums of the iterate's, the direction's and the scratch target; 3 c = S G0 x [m]; 4 mid_in; 5 mid_out;
 * 6 [w; the segment sums of G0 w]; 7 the norm target's T G0 u [m]; 8 its scalar slot on the device and in the pinned mirror [2]; 9 S [m m]; 10 T' [m m] -> host[*len],
 * *len <= cap.
 * pmh_op_penalized_test_norm_target: Gu != NULL: T G0 u of every emitted iterate -> Gu (device, m doubles), its squared norm -> scalar slot `slot`; Gu == NULL:
 * *ready = whether both hold the values of the device vector u (one small launch forms them where the sums wait and no application followed); synchronises.
 * pmh_op_penalized_test_mult_epi2: pmh_op_penalized_test_mult_epi with every operand: kind 0, 1 (P1: x = p, y = Ap, operands g, xx, lb, ub; block partials in rows
 * 4..6) or 2 (gradient split: operands b, lb, ub, astol; rows 0..3), in_slot 0 (the chain forms G0 x itself), 1 / 2 (the iterate's / the direction's target holds
 * it).  partials_*_host [8][2048]: in, the block partials on the device / in the pinned copy before; out, afterwards.  *nblocks: blocks the last kernel wrote;
 * *replayed: 1 where the last kernel ran alone.  An operator that is not on the chain is taken with in_slot = 0 and same_input = 0 (else PMH_ERR_SUP): its product
 * with the vector phase in its last kernel as a caller without a pinned copy gets it (device rows only, *nblocks = the workgroups of the streaming grid);
 * PMH_ERR_SUP where the product has no such kernel as it is configured.
 * pmh_op_penalized_test_form: *form = the product the next application takes under the current knobs: 0 the one-row equality folded into the SVM operator, 1 the
 * dual-space chain, 2 the one-launch projector (k_gt_fused1d), 3 the 10-launch form (k_gt_fused / k_gt_fused1), 4 the 12-launch form with the dense (G G')^-1
 * (k_gt_dual1), 5 the plain sequence.
 * pmh_op_penalized_test_aux_normG: T G0 u -> Gu (device, m doubles) and its squared norm -> scalar slot `slot`, armed = 0 by the projector's own two launches, armed = 1
 * as a request riding on the product y = A x (*served = 1 where the product took it; x, y device vectors).  scal[2]: in, what the device slot and its pinned mirror
 * hold before; out, afterwards.  Synchronises. */
int pmh_op_test_create_staged(pmh_csr gather, pmh_csr middle, pmh_csr scatter, pmh_op *op);
int pmh_op_penalized_test_chain_info(pmh_op op, long long info[10]);
int pmh_op_penalized_test_chain_read(pmh_op op, int what, int cap, double *host, int *len);
int pmh_op_penalized_test_norm_target(pmh_op op, double *Gu, int slot, const double *u, int *ready);
int pmh_op_penalized_test_mult_epi2(pmh_op op, int kind, int same_input, int in_slot, const double *x, const double *b, const double *g, const double *xx, const double *lb,
                                    const double *ub, double astol, double *y, double *gf, double *p, double *partials_dev_host, double *partials_pinned_host, int *nblocks,
                                    int *replayed);
int pmh_op_penalized_test_form(pmh_op op, int *form);
int pmh_op_penalized_test_aux_normG(pmh_op op, int armed, const double *u, double *Gu, int slot, const double *x, double *y, double scal[2], int *served);
/* ---- 3x3-block product test entries (csrc/bsr.hip: the conversion as the V-cycle and K^+ call it, and one launch of k_bsr3; nothing inside the solvers changes) ----
 * pmh_bsr3_test_create: the 3x3-block device copy of the square CSR A with entries kept in `storage` (0 fp64, 1 fp32, 2 fp16 scaled by a power of two, fp32
 * arithmetic), tiles of `tile` blocks (512; any other value: 1024) and nrep_hint congruent diagonal blocks (believed only after an entry-by-entry comparison).
 * *B = NULL with PMH_SUCCESS where the conversion declines: n == 0 or n % 3 != 0, a block row with more blocks than a tile, blocks mostly empty
 * (9 nblocks > 2 nnz + 64).
 * pmh_bsr3_test_info: info = {n, block rows, tiles, blocks per tile (512 / 1024), replicas, blocks, padded blocks, W = blocks per vector load (2 fp64, 4 fp32 / fp16)};
 * block rows, tiles, blocks and padded blocks describe ONE replica.  *scale (or NULL): the fp16 scale (1 otherwise; 1 for a matrix without entries).
 * pmh_bsr3_test_mult_epi: one launch with the epilogue `epi` on device vectors of n entries -- double for fp64 storage, float otherwise (z64: always double):
 *   0 NONE y = A x;  1 ADD y = y1 + A x;  2 SUB y = A x - y1;  10 PRE y = c0 x + c2 dinv (y1 - A x);  11 POST1 r = dinv (y1 - A x), d = c0 r, y = x + d;
 *   12 POST2 y += c1 x + c2 (r - dinv A x), z64 (or NULL) = (double)y.
 * halt != 0: the launch sees a device flag set to 1 and changes nothing.  Synchronises.  PMH_ERR_ARG for an operand the epilogue needs and does not get, and for
 * y (POST1: also r, d; POST2: also z64) == x: no variant may write the vector it gathers from. */
int pmh_bsr3_test_create(pmh_csr A, int storage, int tile, int nrep_hint, void **B);
int pmh_bsr3_test_info(void *B, long long info[8], double *scale);
int pmh_bsr3_test_mult_epi(void *B, int epi, const void *x, void *y, const void *y1, const void *dinv, void *r, void *d, double *z64, double c0, double c1, double c2, int halt);
int pmh_bsr3_test_destroy(void *B);
/* ---- orbit GEMM test entries (csrc/fshared.hip: the plan as the assembly makes it and the launches of the apply; nothing inside the kernels, the plan or the solvers
 * changes) ----
 * pmh_fexplicit_test_load_class: PMH_FX_CLASS_ORBIT, after the symmetries of every class with touched dofs are set: plans the GEMM (as the assembly does) and stores
 * the rows of class cls's orbit representatives from the HOST matrix W_host (n_c x n_c, row-major, in the numbering of pmh_fexplicit_class_union) -- any matrix that
 * is invariant under the class's signed permutations; no K^+ solve, no symmetry-adapted form (callers keep the knob orbit_adapted at 0).  Once every class with touched
 * dofs is loaded the operator counts as assembled: pmh_fexplicit_dense_mult, _mult and _get_block work as after pmh_fexplicit_assemble.  PMH_ERR_ARG for another
 * storage or a class out of range, PMH_ERR_STATE where a class with touched dofs has no symmetries.
 * pmh_fexplicit_orbit_plan_info: what the plan decided for class cls and what the apply launches, info = {0 n_c, 1 ld, 2 slots per multivector record, 3 groups,
 * 4 offset of the class in the multivector numbering (entry: offset + group ld slots + position slots + slot), 5 operations, 6 padded operations, 7 representatives M,
 * 8 row tile, 9 padded rows, 10 row tiles, 11 column tile TN (128 / 64), 12 TNW (48: the 48-column kernel of one-block classes, else 0), 13 k segments, 14 chunks of
 * 16 k positions, 15 units (group, row tile, segment), 16 units with chunks on this rank, 17 largest split count of a unit, 18 workgroups, 19 workgroups with two or
 * more items, 20 launch: 0 the single-class kernel, 1 a table-driven launch per class, 2 one merged table-driven launch over all classes, 21 finishing: 0 k_fxo_fin per
 * class, 1 k_fxo_fin_all, 22 / 23 this rank's range of the representatives}.  PMH_ERR_STATE before there is a plan. */
int pmh_fexplicit_test_load_class(pmh_fexplicit E, int cls, const double *W_host);
/* pmh_fexplicit_assemble_window (tests of the set-up's batch windows, which the library itself reaches only through the probe of pmh_feti_contact_solve): pmh_fexplicit_assemble
 * restricted to the batches [begin, end) of its plan, in the order and with the columns the whole set-up gives them; call it window after window.  Out: the plan's batches (the
 * self-check of a set-up by symmetry is the last one) and K^+ solves, and whether this window reached the last batch -- only then the operator counts as assembled. */
int pmh_fexplicit_assemble_window(pmh_fexplicit E, pmh_matinv solver, int nslots, const int *slot_class, const int *block_class, double rtol, int max_it, int begin, int end, int *nbatch,
                                  long long *nsolves, int *complete);
int pmh_fexplicit_orbit_plan_info(pmh_fexplicit E, int cls, long long info[24]);
/* ---- test entries of the other four storages (PMH_FX_FULL, _SYM: csrc/fexplicit.hip; PMH_FX_CLASS, _CLASS_SYM: csrc/fshared.hip); no kernel, launch or table of the
 * apply changes, called by nothing inside the solvers.  unit: the block (FULL / SYM) or the class (CLASS / CLASS_SYM); matrix numbering: Gamma_b resp.
 * pmh_fexplicit_class_union.
 * pmh_fexplicit_test_load_rows: the rows [row0, row0 + nrows) of the unit's matrix from HOST memory (nrows rows of n doubles), stored by the launches of the set-up's
 * own plan -- fx_extract_row (FULL, CLASS), k_fx_extract_tiled with the band's column cap (SYM), k_fxs_extract_sym (CLASS_SYM) or, in a class with symmetries,
 * k_fxs_extract_symg for every owned row of the orbit of a loaded representative (other rows of that class are ignored) -- from a device vector in block-relative dof
 * numbering; no K^+ solve.  Rows outside this rank's stripe are skipped as in the assembly.  mode 1 (FULL / SYM, row0 = 0, nrows = n, not striped): the n x n matrix
 * goes through k_fx_store_sym instead, (S + S') / 2 as the Dirichlet preconditioner stores its blocks.  Once every row of every unit with touched dofs was handed over
 * the operator counts as assembled (pmh_fexplicit_dense_mult, _mult, _get_block); later loads overwrite.
 * pmh_fexplicit_test_info (reads state only): info = {0 storage, 1 n, 2 ld, 3 bands (SYM: super bands of 128 rows; CLASS: row groups of 32; CLASS_SYM: mega bands of
 * 1024 rows), 4 bands this rank owns, 5 .. 9 by storage, 10 offset of the unit in the compressed / multivector numbering, 11 its offset in the dense allocation,
 * 12 groups of 8 blocks (class storages), 16 + k: band k < 64 is owned}.  FULL: 5 rows per wave, 6 workgroups.  SYM: 5 tile columns per workgroup of k_fx_symv (the
 * segment length in use), 6 the length the rule fx_pick_seg gives, 7 workgroups of k_fx_symv, 8 of k_fx_symv_fin, 9 segments of the unit's last super band.  CLASS:
 * 5 row segments of k_fxs_gemm8, 6 / 7 this rank's rows [r0, r1), 8 workgroups.  CLASS_SYM: 5 workgroups of k_fxs_symm8, 6 its work items, 7 the most items a
 * (group, mega band) of the class is cut into, 9 super bands of 256 rows.
 * pmh_fexplicit_test_set_seg: PMH_FX_SYM, seg in {2, 4, 8, 16}: rebuilds the launch table of k_fx_symv with that segment length (the buffers are sized for the shortest);
 * 0 restores the rule.  pmh_fexplicit_test_read_storage: count doubles of the dense allocation from `offset` on, pads included, to HOST memory. */
int pmh_fexplicit_test_load_rows(pmh_fexplicit E, int unit, int row0, int nrows, const double *rows_host, int mode);
int pmh_fexplicit_test_info(pmh_fexplicit E, int unit, long long info[80]);
int pmh_fexplicit_test_set_seg(pmh_fexplicit E, int seg);
int pmh_fexplicit_test_read_storage(pmh_fexplicit E, long long offset, long long count, double *out_host);
/* pmh_fexplicit_orbit_adapted_info: what the block products (k_fxa_prod) run for class cls while it applies W_c in the symmetry-adapted basis (pmh_fexplicit_orbit_adapted);
 * called by nothing inside the solvers.  20 entries per irrep i = 0 .. 9 at info + 20 i: {0 d, 1 m, 2 k steps of 8 columns nks, 3 blocks of 16 output rows, 4 blocks of 16
 * columns, 5 .. 8 work items of 1 / 2 / 3 / 4 blocks of columns, 9 .. 12 trips of waves 0 .. 3 on an item of 1 or 2 blocks, 13 .. 16 on an item of 3 or 4, 17 / 18 k steps
 * per trip of the two kinds (a wave's k range is its trips in increasing order), 19 whether the class's transforms are the narrow kernels (k_fxa_narrow; the same in
 * every irrep's entry)}.  PMH_ERR_ARG for a storage other than PMH_FX_CLASS_ORBIT or a class out of range, PMH_ERR_STATE where the class is on the GEMM. */
int pmh_fexplicit_orbit_adapted_info(pmh_fexplicit E, int cls, long long info[200]);
/* pmh_fexplicit_orbit_adapted_transform (tests; called by nothing inside the solvers): ONE transform of class cls as the application launches it.  inverse = 0: in is a
 * multivector in the numbering of pmh_fexplicit_dense_mult (zero off the touched sets), out receives X^ = U' X as n_c x NC doubles, entry (basis function r in the numbering
 * of pmh_orbit_basis, column = group * 8 + slot) at r * NC + column, NC = 8 * groups.  inverse = 1: in is Y^ in that order, out receives the multivector Y = U Y^ (zero where
 * no block touches).  Device arrays.  PMH_ERR_STATE where the class is on the GEMM. */
int pmh_fexplicit_orbit_adapted_transform(pmh_fexplicit E, int cls, int inverse, const double *in, double *out);
/* U = K^+ F for 8 columns per block at once: F, U device arrays of 8 n doubles, entry (dof i, column r) at i * 8 + r; K, the V-cycle (pmh_matinv_set_pc_mg), the kernel
 * basis (pmh_matinv_set_nullspace: K^+ = P_R K^- P_R) and the tolerances are the solver's own; every (block, column) pair converges by its own test.  PMH_ERR_SUP where
 * the multi-right-hand-side kernels do not apply (K without regular 3 x 3 blocks, a V-cycle other than the fused fp32 one, the left generalised inverse). */
int pmh_matinv_mult_multi(pmh_matinv M, const double *F, double *U, int *max_iterations /* or NULL */);
/* pmh_matinv_mult (MatMult_Inv, matinv.c:734-743) itself takes these kernels when the solver has exactly 8 congruent blocks (verified entry by entry by pmh_matinv_enable_bsr3)
   and the fused fp32 V-cycle: the 8 blocks' vectors are the 8 columns of ONE block.  *active: whether the next application will (knob "kplus_mv" / PMH_NO_KPLUS_MV for the A/B). */
int pmh_matinv_multi_rhs_active(pmh_matinv M, int *active);
/* Test entries of the block CG (tests/test_gpu_cg_paths.py; called by nothing inside the solvers, and they launch nothing).
 * pmh_matinv_test_info: the state the last pmh_matinv_mult left on the device.  info = {0 workgroups per block of the vector kernels (wgs), 1 the product: 0 CSR, 1 3 x 3
 * blocks, 2 the 8-column ELL copy, 2 the solver: 1 one column a block, 8 eight columns a block, 9 eight congruent blocks as the columns of one, 3 nactive, 4 done, 5 entries =
 * blocks (one column) or columns, 6 the largest iteration count the host read, 7 operator products so far}.  For entry e < min(entries, cap): scal[2 e] = {rz, tol}, ints[2 e]
 * = {active, its} of the parity written last (the one with the larger its; a carried frozen state makes the two equal).  scal / ints may be NULL.
 * pmh_matinv_test_mv_*: the solver of pmh_matinv_mult_multi with its handle kept from one application to the next (_mult synchronises), and the same info for it. */
int pmh_matinv_test_info(pmh_matinv M, long long info[8], int cap, double *scal, int *ints);
int pmh_matinv_test_mv_create(pmh_matinv M, void **V);
int pmh_matinv_test_mv_mult(void *V, const double *F, double *U);
int pmh_matinv_test_mv_info(void *V, long long info[8], int cap, double *scal, int *ints);
int pmh_matinv_test_mv_destroy(void *V);

#ifdef __cplusplus
}
#endif
#endif /* PERMON_HIP_H */
