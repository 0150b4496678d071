// QPS MPGP on gfx950: QPSSetup_MPGP / QPSSolve_MPGP (src/qps/impls/mpgp/mpgp.c:359-650).
//
// Two drivers behind one entry point:
//  * solve_unfused(): the reference's operation sequence, one device kernel per PETSc Vec/Mat/QPC call
//    (every expansion type x step-length rule, fallback, fallback2).  It exists so that every variant of
//    the reference is available and so that each op-table slot is exercised exactly as PERMON calls it.
//  * solve_fused(): the default variant (std expansion, fixed length, no fallback): the ~25 passes of an
//    iteration collapse into the phases of SURVEY 8d --
//      P1  Ap = A p  with  p'Ap, g'p, QPCFeas fused into the SpMV epilogue          (B_spmv + 24 n bytes)
//      P2  x -= a p, g -= a Ap, gradient split, Ap'gf, |gP|^2, |gc|^2, |gf|^2       (64 n bytes)
//      P3  p = gf - beta p                                                            (24 n bytes)
//    gP, gc, gr are never stored (gc / gr are recomputed inside the rare proportioning / expansion
//    kernels).  Step lengths are read by the kernels from device scalars; the host only decides the step
//    TYPE, and the next iteration's SpMV is enqueued speculatively before the host reads the scalars.
// Both produce the same iterates up to reduction-order rounding; tests compare them with the CPU oracle.
#include <cmath>
#include <string>
#include <vector>

#include "pmh_internal.h"
#include "reduce.h"
#include "box_inline.h"
#include "emit_inline.h"

#define GRID_STRIDE(i, n) for (long long i = (long long)blockIdx.x * PMH_BLOCK + threadIdx.x; i < (n); i += (long long)gridDim.x * PMH_BLOCK)
// the entries of a vector kernel: grid-strided over workgroups of 256 threads, or -- EMIT variants, which end with pmh_emit_tail -- thread t of the 1024-thread
// workgroup b owns entry 1024 b + t
#define VEC_ENTRIES(i, n) \
  for (long long i = EMIT ? ((long long)blockIdx.x * PMH_EMIT_TILE + threadIdx.x) : ((long long)blockIdx.x * PMH_BLOCK + threadIdx.x); i < (n); i += EMIT ? (long long)(n) : (long long)gridDim.x * PMH_BLOCK)
#define VEC_BOUNDS __launch_bounds__(EMIT ? PMH_EMIT_TILE : PMH_BLOCK)

// scalar slots
#define S_PAP 8
#define S_GP 9
#define S_FEAS 10
#define S_APGF 16
#define S_GP2 17
#define S_GC2 18
#define S_GF2 19
#define S_TMP 24

// Which partial sums of the context's block partials (ctx->d_partials, pinned copy ctx->h_partials) are still owed, and by whom.  A phase or an operator says
// what it left (note); whoever reads the scalars next on the device has them finalised there (settle); the host adds the pinned rows itself after its next wait
// (host_sums).  The op and slot tables of both groups are OWED_OPS / OWED_SLOTS and nowhere else.
namespace { // (this file's own: the library exports no symbol of it)
struct owed_sums {
  enum { NONE = 0, DEVICE, HOST }; // nothing owed / a finalising launch / the host's sum of the pinned rows
  // SPLIT: rows 0..3 (Ap'gf, |gP|^2, |gc|^2, |gf|^2) -> S_APGF..S_GF2, left by a split or step kernel; P1: rows 4..6 (p'Ap, g'p, QPCFeas) -> S_PAP..S_FEAS
  enum { SPLIT = 1, P1 = 2 };
  struct rows {
    int owed = NONE, nb = 0; // nb: the block partials per row
  } split, p1;

  void clear() { split = rows(), p1 = rows(); }
  void note(int group, int owed, int nb) { (group == SPLIT ? split : p1) = (owed == HOST && nb <= 0) ? rows() : rows{owed, nb}; } // (no block, no sum for the host)
  // the group's finalising launch, at once, of the rows that start at `row` (halt / post: the speculative chain's words, pmh_finalize_partials)
  static int finalize(pmh_ctx ctx, int group, int row, int nb, const int *halt = nullptr, int *post = nullptr);
  // Finalising launches for what is owed of `groups` (SPLIT | P1) on the device -- host_too: and for what was left to the host, where the next reader is a kernel
  // that takes the scalars from d_scal.  Both groups owed device-side over the same blocks, scalars not row-distributed: ONE launch of seven rows, every quantity
  // reduced as on its own.  (Row-distributed scalars are never deferred: their finalising launch is completed across the ranks, in the order the phases ran.)
  int settle(pmh_ctx ctx, int groups, bool host_too = false, const int *halt = nullptr, int *post = nullptr);
  // after a wait on the stream: the sums the EMIT kernels / the operator's last kernel left to the host (the role of k_finalize) -> h_scal
  void host_sums(pmh_ctx ctx);
};
} // namespace

struct pmh_mpgp_s {
  pmh_ctx       ctx = nullptr;
  pmh_op        A   = nullptr;
  pmh_csr       csr = nullptr;
  int           n   = 0;
  const double *b   = nullptr;
  double       *x   = nullptr;
  const double *lb = nullptr, *ub = nullptr;
  pmh_mpgp_opts o;
  // QPS_MPGP state
  double  alpha = 0.0, alpha_user = 0.0, maxeig = 0.0;
  int     expproject = 1; // mpgp.c:839
  double *work[10]   = {};
  int     nwork      = 0;
  // convergence
  pmh_converged_fn cvg      = nullptr;
  void            *cvg_user = nullptr;
  double           norm_rhs = 0.0, ttol = 0.0, norm_rhs_div = 0.0;
  int              cvg_setup = 0;
  // optional: enqueues what the injected convergence test will read, BEFORE the host waits for the step's scalars (one round trip instead of two)
  int (*pre_test)(void *) = nullptr;
  void *pre_test_user     = nullptr;
  // optional: called right before the speculative Ap = A p of the NEXT iteration is enqueued (the iterate is final then): SMALXE lets its ||B u|| ride on that
  // product
  int (*pre_p1)(void *) = nullptr;
  void *pre_p1_user     = nullptr;
  // set by the convergence test: rnorm / (the threshold it has to fall below), 0 = unknown -- how close the NEXT test is to ending the solve
  double cvg_margin = 0.0;
  // work[3] already holds A x - b for the x and b the next solve starts from (pmh_mpgp_set_gradient_valid): the fused driver skips its first product
  int g_valid = 0;
  int epi_ok  = -1; // 1: the operator folds the vector phases into its last kernel (pmh_op_s::mult_epi), 0: it does not, -1: not asked yet
  // the partial sums the phases and the operator have left behind and nobody has summed yet
  owed_sums owed;
  // fused dual-space chain (pmh_op_s::emit_begin): the operator holds G0 x (0) / G0 p (1) of the CURRENT x / p, emitted by the kernel that wrote them
  bool cx[2] = {false, false};
  // the operator's last application was the gradient at x and nothing has written x since (every write of x and every other application clears it): a caller
  // that multiplies x again may say so (pmh_op_s::mult_same_input).  first_applied: the caller's word that the NEXT solve's first gradient is such a repeat
  bool x_applied     = false;
  int  first_applied = 0;
  // results
  double rnorm = 0.0, gfnorm = 0.0, gcnorm = 0.0;
  int    iteration = 0, reason = 0;
  int    nmv = 0, ncg = 0, nexp = 0, nprop = 0, nfinc = 0, nfall = 0;
  char   step           = ' ';
  int    fallback_state = 0;
  // monitor
  std::vector<char>   t_step;
  std::vector<double> t_gp, t_gf, t_gc, t_alpha;
  // speculative device-side CG chain
  int    *d_ctl = nullptr, *h_ctl = nullptr;
  double *d_ring = nullptr, *h_ring = nullptr;
};

// --------------------------------------------------------------------------------------------------------------------
// device helpers: the box predicates of qpcbox.c restated per element
// --------------------------------------------------------------------------------------------------------------------
// (the box predicates pmh_box_split / pmh_box_reduced / pmh_box_feas and the per-entry terms of the two vector phases, pmh_p1_terms / pmh_split_terms:
// box_inline.h; a workgroup's accumulators to its row of block partials, write_partials: reduce.h)

// gradient split + norms (+ p = gf): after the initial gradient and after an expansion step
// (MPGPGrads mpgp.c:198-223 + VecCopy(gf,p) :507/:615 + the three reductions of :514-521)
template <bool EMIT>
__global__ VEC_BOUNDS void k_split_setp(long long n, const double *__restrict__ x, const double *__restrict__ g, const double *__restrict__ lb, const double *__restrict__ ub, double astol, double *__restrict__ gf, double *__restrict__ p, double *__restrict__ partials, int ld, pmh_emit_args ea, double *__restrict__ h_partials)
{
  __shared__ double lds[PMH_BLOCK / 64];
  double            acc[4] = {0.0, 0.0, 0.0, 0.0}, pv = 0.0, zv = 0.0;
  pmh_emit_regs     R;
  if (EMIT) pmh_emit_prefetch(ea, R);
  VEC_ENTRIES(i, n)
  {
    const double f = pmh_split_terms(acc, x[i], g[i], lb, ub, i, astol);
    gf[i]          = f;
    p[i]           = f;
    pv             = f;
  }
  write_partials<4, EMIT>(acc, lds, partials, ld, h_partials);
  if (EMIT) pmh_emit_tail(ea, R, zv, pv); // the segment sums of G0 p for the p = gf just written
}

// device control words of the speculative CG chain
enum { CTL_HALT = 0, CTL_ITER, CTL_NCG, CTL_BASE, CTL_NWORDS };

struct pmh_spec_args { // constants of one solve, passed by value
  int    *ctl;   // device: [halt, iteration, ncg, base]
  double *ring;  // device: per device-side iteration (|gP|^2, |gf|^2, |gc|^2) for the monitor trace
  int     ring_cap;
  int     max_it;
  double  ttol, divtol_rhs, gamma2;
};

// P2: CG / proportioning update.  acg = (g'p)/(p'Ap) from device scalars (mpgp.c:541-543, :628-630);
// x -= acg p; g -= acg Ap (:553-554 / :633-634); split (:555 / :635); Ap'gf for beta (:558); norms.
// SPEC: the kernel first evaluates, from the device scalars alone, everything the host loop would check
// at the top of this iteration -- QPSConvergedDefault (qps.c:688-712), proportionality (mpgp.c:535) and
// acg <= afeas (mpgp.c:547).  If this is a plain CG step it is taken without any host round trip; otherwise
// the chain halts with the state untouched and the host driver takes this iteration.
template <bool SETP, bool SPEC, bool EMIT = false>
__global__ VEC_BOUNDS void k_step_update(long long n, const double *__restrict__ scal, pmh_spec_args sa, double *__restrict__ x, double *__restrict__ g, double *__restrict__ p, const double *__restrict__ Ap, const double *__restrict__ lb, const double *__restrict__ ub, double astol, double *__restrict__ gf, double *__restrict__ partials, int ld, pmh_emit_args ea, double *__restrict__ h_partials, double acg_host, int nb_p1)
{
  __shared__ double lds[PMH_BLOCK / 64];
  double            acg;
  pmh_emit_regs     R;
  if (EMIT) pmh_emit_prefetch(ea, R);
  // no finalising launch ran: acg from the host (it has read p'Ap, g'p) or -- proportioning, taken without a host wait -- from the P1 block partials (rows 4,
  // 5)
  if (EMIT) {
    acg = acg_host;
    if (nb_p1 > 0) acg = pmh_sum_block_partials(partials + (size_t)5 * ld, nb_p1) / pmh_sum_block_partials(partials + (size_t)4 * ld, nb_p1);
  } else {
    acg = scal[S_GP] / scal[S_PAP];
  }
  if (SPEC) {
    if (sa.ctl[CTL_HALT]) return;
    const int    it  = sa.ctl[CTL_ITER];
    const double gP2 = scal[S_GP2], gc2 = scal[S_GC2], gf2 = scal[S_GF2], rnorm = sqrt(gP2);
    bool         go;
    go = (it <= sa.max_it) && (rnorm > sa.ttol) && (rnorm < sa.divtol_rhs); // NaN fails every comparison -> halt
    go = go && (gc2 <= sa.gamma2 * gf2) && (acg <= scal[S_FEAS]) && (it - sa.ctl[CTL_BASE] < sa.ring_cap);
    if (!go) {
      if (blockIdx.x == 0 && threadIdx.x == 0) sa.ctl[CTL_HALT] = 1; // every workgroup reaches the same verdict
      return;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      const int k        = it - sa.ctl[CTL_BASE];
      sa.ring[3 * k]     = gP2;
      sa.ring[3 * k + 1] = gf2;
      sa.ring[3 * k + 2] = gc2;
    }
  }
  const double ma     = -acg;
  double       acc[4] = {0.0, 0.0, 0.0, 0.0}, xv = 0.0, pv = 0.0;
  VEC_ENTRIES(i, n)
  {
    double api = Ap[i];
    double xi  = x[i] + ma * p[i];
    double gi  = g[i] + ma * api;
    double f, c;
    pmh_box_split(xi, gi, lb, ub, i, astol, f, c);
    x[i]  = xi;
    g[i]  = gi;
    gf[i] = f;
    if (SETP) p[i] = f;
    xv = xi, pv = f;
    double gPi = f + c; // (pmh_split_terms written out: through the helper three instantiations take two more registers)
    acc[0] += api * f;
    acc[1] += gPi * gPi;
    acc[2] += c * c;
    acc[3] += f * f;
  }
  write_partials<4, EMIT>(acc, lds, partials, ld, h_partials);
  if (EMIT) pmh_emit_tail(ea, R, xv, pv); // the segment sums of G0 x (and of G0 p where p = gf was set)
}

// P3: p = gf - bcg p, bcg = (Ap'gf)/(p'Ap) (mpgp.c:558-560: VecAYPX(p,-bcg,gf))
template <bool EMIT>
__global__ VEC_BOUNDS void k_dir_update(long long n, const double *__restrict__ scal, const int *__restrict__ halt, const double *__restrict__ gf, double *__restrict__ p, pmh_emit_args ea, const double *__restrict__ partials, int nb, double pAp_host)
{
  if (halt && *halt) return;
  pmh_emit_regs R;
  if (EMIT) pmh_emit_prefetch(ea, R);
  // EMIT: Ap'gf from the block partials k_step_update just left (row 0: no finalising launch ran), p'Ap from the host
  double       bcg = EMIT ? pmh_sum_block_partials(partials, nb) / pAp_host : scal[S_APGF] / scal[S_PAP];
  const double mb  = -bcg;
  double       pv = 0.0, zv = 0.0;
  VEC_ENTRIES(i, n) p[i] = pv = gf[i] + mb * p[i];
  if (EMIT) pmh_emit_tail(ea, R, zv, pv);
}

// proportioning direction p = gc (mpgp.c:623), gc recomputed from x, g
template <bool EMIT>
__global__ VEC_BOUNDS void k_prop_dir(long long n, const double *__restrict__ x, const double *__restrict__ g, const double *__restrict__ lb, const double *__restrict__ ub, double astol, double *__restrict__ p, pmh_emit_args ea)
{
  double        pv = 0.0, zv = 0.0;
  pmh_emit_regs R;
  if (EMIT) pmh_emit_prefetch(ea, R);
  VEC_ENTRIES(i, n)
  {
    double f, c;
    pmh_box_split(x[i], g[i], lb, ub, i, astol, f, c);
    p[i] = pv = c;
  }
  if (EMIT) pmh_emit_tail(ea, R, zv, pv);
}

// expansion (std direction, fixed length; MPGPExpansion_Std mpgp.c:299-323):
// x -= afeas p; g -= afeas Ap; split; gr; x -= alpha gr.  g is not stored: it is recomputed as A x - b next.
template <bool EMIT>
__global__ VEC_BOUNDS void k_expansion_std(long long n, double afeas, double alpha, double *__restrict__ x, const double *__restrict__ g, const double *__restrict__ p, const double *__restrict__ Ap, const double *__restrict__ lb, const double *__restrict__ ub, double astol, pmh_emit_args ea)
{
  const double maf = -afeas, mal = -alpha;
  double       xv = 0.0, zv = 0.0;
  pmh_emit_regs R;
  if (EMIT) pmh_emit_prefetch(ea, R);
  VEC_ENTRIES(i, n)
  {
    double xi = x[i] + maf * p[i];
    double gi = g[i] + maf * Ap[i];
    double f, c;
    pmh_box_split(xi, gi, lb, ub, i, astol, f, c);
    double r = pmh_box_reduced(xi, f, lb, ub, i, alpha);
    x[i] = xv = xi + mal * r;
  }
  if (EMIT) pmh_emit_tail(ea, R, xv, zv);
}

// p'Ap, g'p, QPCFeas for operators without a fused SpMV epilogue (shell operators: F, P F P, A + rho Q ...)
__global__ __launch_bounds__(PMH_BLOCK) void k_p1_dots(long long n, const double *__restrict__ p, const double *__restrict__ Ap, const double *__restrict__ g, const double *__restrict__ x, const double *__restrict__ lb, const double *__restrict__ ub, double *__restrict__ partials, int ld)
{
  __shared__ double lds[PMH_BLOCK / 64];
  double            s[3] = {0.0, 0.0, INFINITY};
  GRID_STRIDE(i, n) pmh_p1_terms(s, p[i], Ap[i], g[i], x, lb, ub, i);
  write_partials<3>(s, {PMH_RED_SUM, PMH_RED_SUM, PMH_RED_MIN}, lds, partials, ld);
}

// three squared norms in one pass (unfused driver: VecNorm(gP), VecDot(gc,gc), VecDot(gf,gf) mpgp.c:514-521)
__global__ __launch_bounds__(PMH_BLOCK) void k_three_norms(long long n, const double *__restrict__ gP, const double *__restrict__ gc, const double *__restrict__ gf, double *__restrict__ partials, int ld)
{
  __shared__ double lds[PMH_BLOCK / 64];
  double            acc[4] = {0.0, 0.0, 0.0, 0.0};
  GRID_STRIDE(i, n)
  {
    double a = gP[i], c = gc[i], f = gf[i];
    acc[1] += a * a;
    acc[2] += c * c;
    acc[3] += f * f;
  }
  write_partials<4>(acc, lds, partials, ld);
}

__global__ __launch_bounds__(PMH_BLOCK) void k_filter(long long n, double *v, double tol)
{
  GRID_STRIDE(i, n) if (fabs(v[i]) < tol) v[i] = 0.0;
}

// objective from gradient f = 1/2 x'(g - b) (QPComputeObjectiveFromGradient qp.c:981-996)
__global__ __launch_bounds__(PMH_BLOCK) void k_obj_from_grad(long long n, const double *__restrict__ x, const double *__restrict__ g, const double *__restrict__ b, double *__restrict__ partials)
{
  __shared__ double lds[PMH_BLOCK / 64];
  double            s = 0.0;
  GRID_STRIDE(i, n) s += x[i] * (-1.0 * b[i] + g[i]);
  s = pmh_block_reduce<PMH_RED_SUM>(s, lds);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// --------------------------------------------------------------------------------------------------------------------
// the phases: one launcher each, called by both drivers and by the test entry (pmh_mpgp_test_phase)
// --------------------------------------------------------------------------------------------------------------------
static int vec_blocks(int n) { return n > 0 ? pmh_vec_grid(n) : 0; }               // grid of the plain kernels
static int emit_blocks(int n) { return (n + PMH_EMIT_TILE - 1) / PMH_EMIT_TILE; } // grid of the EMIT variants

// The one launch of a vector kernel over n entries: the 256-thread grid of pmh_vec_grid, or -- tile: the EMIT variants -- workgroups of PMH_EMIT_TILE threads,
// one entry each.  The arguments are converted to the kernel's own parameter types.
template <typename... P, typename... T>
static int launch(pmh_ctx ctx, int n, bool tile, void (*kern)(long long, P...), T... args)
{
  if (n > 0) hipLaunchKernelGGL(kern, dim3(tile ? emit_blocks(n) : pmh_vec_grid(n)), dim3(tile ? PMH_EMIT_TILE : PMH_BLOCK), 0, ctx->stream, (long long)n, (P)args...);
  PMH_HIP(hipGetLastError());
  return PMH_SUCCESS;
}

// what the phase kernels work on: the reference's work vectors (mpgp.c:6-17) and the box
struct phase_vecs {
  double       *x, *g, *p, *Ap, *gf;
  const double *lb, *ub;
  double        astol;
};

// Each launcher: ea == nullptr is the plain kernel (no emission: g_noea, no pinned copy of the partials, no host scalars), otherwise the tile variant that
// leaves the segment sums *ea asks for (pmh_op_s::emit_begin) and its block partials in the pinned copy as well.  The sums go to rows 0.. of ctx->d_partials.
static pmh_emit_args g_noea;

static int phase_split(pmh_ctx ctx, int n, const phase_vecs &v, const pmh_emit_args *ea) { return launch(ctx, n, ea, ea ? k_split_setp<true> : k_split_setp<false>, v.x, v.g, v.lb, v.ub, v.astol, v.gf, v.p, ctx->d_partials, ctx->partials_cap, ea ? *ea : g_noea, ea ? ctx->h_partials : nullptr); }

// setp: p = gf as well (proportioning); spec: the device-side test of the speculative chain (plain kernel, CG step only).  Tile variant: acg from the host, or
// -- nb_p1 > 0 -- from the P1 block partials.  The one place that chooses among the instantiations of k_step_update
static int phase_step(pmh_ctx ctx, int n, const phase_vecs &v, bool setp, const pmh_spec_args *spec, const pmh_emit_args *ea, double acg_host, int nb_p1)
{
  auto kern = ea ? (setp ? k_step_update<true, false, true> : k_step_update<false, false, true>) : spec ? k_step_update<false, true> : setp ? k_step_update<true, false> : k_step_update<false, false>;
  return launch(ctx, n, ea, kern, ctx->d_scal, spec ? *spec : pmh_spec_args{}, v.x, v.g, v.p, v.Ap, v.lb, v.ub, v.astol, v.gf, ctx->d_partials, ctx->partials_cap, ea ? *ea : g_noea,
                ea ? ctx->h_partials : nullptr, ea ? acg_host : 0.0, ea ? nb_p1 : 0);
}

// tile variant: Ap'gf from the nb block partials of row 0, p'Ap from the host
static int phase_dir(pmh_ctx ctx, int n, const phase_vecs &v, const int *halt, const pmh_emit_args *ea, int nb, double pAp_host) { return launch(ctx, n, ea, ea ? k_dir_update<true> : k_dir_update<false>, ctx->d_scal, halt, v.gf, v.p, ea ? *ea : g_noea, ea ? ctx->d_partials : nullptr, ea ? nb : 0, ea ? pAp_host : 0.0); }

static int phase_prop_dir(pmh_ctx ctx, int n, const phase_vecs &v, const pmh_emit_args *ea) { return launch(ctx, n, ea, ea ? k_prop_dir<true> : k_prop_dir<false>, v.x, v.g, v.lb, v.ub, v.astol, v.p, ea ? *ea : g_noea); }

static int phase_expansion(pmh_ctx ctx, int n, const phase_vecs &v, double afeas, double alpha, const pmh_emit_args *ea) { return launch(ctx, n, ea, ea ? k_expansion_std<true> : k_expansion_std<false>, afeas, alpha, v.x, v.g, v.p, v.Ap, v.lb, v.ub, v.astol, ea ? *ea : g_noea); }

static int phase_p1_dots(pmh_ctx ctx, int n, const phase_vecs &v) { return launch(ctx, n, false, k_p1_dots, v.p, v.Ap, v.g, v.x, v.lb, v.ub, ctx->d_partials, ctx->partials_cap); }
static int phase_three_norms(pmh_ctx ctx, int n, const double *gP, const double *gc, const double *gf) { return launch(ctx, n, false, k_three_norms, gP, gc, gf, ctx->d_partials, ctx->partials_cap); }
static int phase_obj(pmh_ctx ctx, int n, const double *x, const double *g, const double *b) { return launch(ctx, n, false, k_obj_from_grad, x, g, b, ctx->d_partials); }

// --------------------------------------------------------------------------------------------------------------------
// set-up
// --------------------------------------------------------------------------------------------------------------------
extern "C" int pmh_mpgp_default_opts(pmh_mpgp_opts *o)
{
  PMH_ARG(o);
  memset(o, 0, sizeof(*o));
  o->rtol          = 1e-5; // QPSCreate qps.c:73-76
  o->atol          = 1e-50;
  o->divtol        = 1e4;
  o->max_it        = 10000;
  o->alpha_user    = PMH_DECIDE; // QPSCreate_MPGP mpgp.c:827-843
  o->alpha_direct  = 0;
  o->gamma         = 1.0;
  o->maxeig        = PMH_DECIDE;
  o->maxeig_tol    = PMH_DECIDE;
  o->maxeig_iter   = -1;
  o->bchop_tol     = 0.0;
  o->astol         = 10 * 2.220446049250313e-16; // qpc.c:28
  o->exptype       = PMH_EXP_STD;
  o->explengthtype = PMH_EXPLEN_FIXED;
  return PMH_SUCCESS;
}

static int ensure_work(pmh_mpgp s, int i)
{
  if (!s->work[i]) {
    PMH_CHK(pmh_malloc(s->ctx, sizeof(double) * (size_t)s->n, (void **)&s->work[i]));
    PMH_CHK(pmh_memset(s->ctx, s->work[i], 0, sizeof(double) * (size_t)s->n));
  }
  return PMH_SUCCESS;
}

static bool use_fused(pmh_mpgp s)
{
  return !s->o.unfused && s->o.exptype == PMH_EXP_STD && s->o.explengthtype == PMH_EXPLEN_FIXED && !s->o.fallback && !s->o.fallback2;
}

// QPSSetup_MPGP mpgp.c:359-428
extern "C" int pmh_mpgp_create(pmh_ctx ctx, pmh_op A, const double *b, double *x, const double *lb, const double *ub, const pmh_mpgp_opts *o, pmh_mpgp *out)
{
  PMH_ARG(ctx && A && b && x && o && out);
  PMH_ARG(o->exptype >= PMH_EXP_STD && o->exptype <= PMH_EXP_GGR);
  PMH_ARG(o->explengthtype >= PMH_EXPLEN_FIXED && o->explengthtype <= PMH_EXPLEN_BB);
  pmh_mpgp s = new pmh_mpgp_s();
  s->ctx     = ctx;
  s->A       = A;
  s->csr     = A->as_csr();
  s->n       = A->n;
  s->b       = b;
  s->x       = x;
  s->lb      = lb;
  s->ub      = ub;
  s->o       = *o;
  if (s->o.fallback2) s->o.fallback = 0; // mpgp.c:744
  s->fallback_state = s->o.fallback;
  if (s->o.bchop_tol) { // mpgp.c:379-382: VecFilter on the user's bound vectors, in place as in the reference
    if (lb) PMH_CHK(launch(ctx, s->n, false, k_filter, lb, s->o.bchop_tol));
    if (ub) PMH_CHK(launch(ctx, s->n, false, k_filter, ub, s->o.bchop_tol));
  }
  if (s->o.exptype == PMH_EXP_STD && s->o.explengthtype == PMH_EXPLEN_FIXED) s->expproject = 0; // mpgp.c:388
  s->maxeig     = s->o.maxeig;
  s->alpha_user = s->o.alpha_user;
  if (!s->o.alpha_direct) { // QPS_ARG_MULTIPLE mpgp.c:417-422
    if (s->maxeig == PMH_DECIDE) {
      ctx->dist_scalars = s->o.distributed;
      int rc            = pmh_op_max_eigenvalue(A, s->o.maxeig_tol, s->o.maxeig_iter, &s->maxeig, nullptr);
      ctx->dist_scalars = 0;
      if (rc) {
        delete s;
        return rc;
      }
    }
    if (s->alpha_user == PMH_DECIDE) s->alpha_user = 2.0;
    s->alpha = s->alpha_user / s->maxeig;
  } else {
    s->alpha = s->alpha_user;
  }
  *out = s;
  return PMH_SUCCESS;
}

extern "C" int pmh_mpgp_destroy(pmh_mpgp s)
{
  if (!s) return PMH_SUCCESS;
  for (int i = 0; i < 10; i++)
    if (s->work[i]) pmh_free(s->ctx, s->work[i]);
  if (s->d_ctl) pmh_free(s->ctx, s->d_ctl);
  if (s->d_ring) pmh_free(s->ctx, s->d_ring);
  if (s->h_ctl) hipHostFree(s->h_ctl);
  if (s->h_ring) hipHostFree(s->h_ring);
  delete s;
  return PMH_SUCCESS;
}

// internal (SMALXE): f is called before the host waits for the scalars of a step, with the iterate already updated; what it enqueues is complete when the
// injected convergence test runs
int pmh_mpgp_set_pre_test_hook(pmh_mpgp s, int (*f)(void *), void *user)
{
  PMH_ARG(s);
  s->pre_test = f, s->pre_test_user = user;
  return PMH_SUCCESS;
}

int pmh_mpgp_set_pre_p1_hook(pmh_mpgp s, int (*f)(void *), void *user)
{
  PMH_ARG(s);
  s->pre_p1 = f, s->pre_p1_user = user;
  return PMH_SUCCESS;
}

extern "C" int pmh_mpgp_set_convergence_test(pmh_mpgp s, pmh_converged_fn f, void *user)
{
  PMH_ARG(s);
  s->cvg      = f;
  s->cvg_user = user;
  return PMH_SUCCESS;
}

extern "C" int pmh_mpgp_set_tolerances(pmh_mpgp s, double rtol, double atol, double divtol, int max_it)
{
  PMH_ARG(s);
  s->o.rtol    = rtol;
  s->o.atol    = atol;
  s->o.divtol  = divtol;
  s->o.max_it  = max_it;
  s->cvg_setup = 0;
  return PMH_SUCCESS;
}

// "QPSMPGPSetOperatorMaxEigenvalue_MPGP_C" mpgp.c:107-115 (then QPSSetup_MPGP recomputes alpha :417-422)
extern "C" int pmh_mpgp_set_operator_max_eigenvalue(pmh_mpgp s, double maxeig)
{
  PMH_ARG(s && (maxeig >= 0 || maxeig == PMH_DECIDE));
  s->maxeig = maxeig;
  if (!s->o.alpha_direct) {
    if (s->maxeig == PMH_DECIDE) PMH_CHK(pmh_op_max_eigenvalue(s->A, s->o.maxeig_tol, s->o.maxeig_iter, &s->maxeig, nullptr));
    s->alpha = s->alpha_user / s->maxeig;
  }
  return PMH_SUCCESS;
}

// "QPSMPGPUpdateMaxEigenvalue_MPGP_C" mpgp.c:119-143
extern "C" int pmh_mpgp_update_max_eigenvalue(pmh_mpgp s, double maxeig_update)
{
  PMH_ARG(s);
  if (maxeig_update == 1.0) return PMH_SUCCESS; // mpgp.c:1007
  s->maxeig = s->maxeig * maxeig_update;
  if (!s->o.alpha_direct) s->alpha = s->alpha / maxeig_update;
  return PMH_SUCCESS;
}

extern "C" int pmh_mpgp_get_current_step_type(pmh_mpgp s, char *step)
{
  PMH_ARG(s && step);
  *step = s->step;
  return PMH_SUCCESS;
}

extern "C" int pmh_mpgp_reset_statistics(pmh_mpgp s)
{
  PMH_ARG(s);
  s->ncg = s->nexp = s->nmv = s->nprop = 0; // mpgp.c:659-662 (nfinc/nfall are not reset there)
  return PMH_SUCCESS;
}

// QPSConvergedDefaultSetUp qps.c:718-731
static int converged_default_setup(pmh_mpgp s)
{
  if (s->cvg_setup) return PMH_SUCCESS;
  PMH_CHK(pmh_vec_norm2(s->ctx, s->n, s->b, &s->norm_rhs));
  s->ttol         = fmax(s->o.rtol * s->norm_rhs, s->o.atol);
  s->norm_rhs_div = s->norm_rhs;
  s->cvg_setup    = 1;
  return PMH_SUCCESS;
}

// QPSConvergedDefault qps.c:675-714
static int converged_default(pmh_mpgp s)
{
  PMH_CHK(converged_default_setup(s));
  s->reason = PMH_CONVERGED_ITERATING;
  if (s->iteration > s->o.max_it) { // strict, qps.c:688
    s->reason = PMH_DIVERGED_ITS;
    return PMH_SUCCESS;
  }
  if (std::isnan(s->rnorm) || std::isinf(s->rnorm)) s->reason = PMH_DIVERGED_NANORINF;
  else if (s->rnorm <= s->ttol) s->reason = (s->rnorm < s->o.atol) ? PMH_CONVERGED_ATOL : PMH_CONVERGED_RTOL;
  else if (s->rnorm >= s->o.divtol * s->norm_rhs_div) s->reason = PMH_DIVERGED_DTOL;
  s->cvg_margin = (s->iteration >= s->o.max_it) ? 1e-300 : s->rnorm / fmax(s->ttol, 1e-300);
  return PMH_SUCCESS;
}

// one line of QPSMonitorDefault_MPGP (mpgp.c:21-34)
static void monitor_push(pmh_mpgp s, double gp, double gf, double gc)
{
  if (!s->o.monitor) return;
  s->t_step.push_back(s->step);
  s->t_gp.push_back(gp);
  s->t_gf.push_back(gf);
  s->t_gc.push_back(gc);
  s->t_alpha.push_back(s->alpha);
}

// monitor (mpgp.c:524-528) + convergence test (mpgp.c:531)
static int test_convergence(pmh_mpgp s)
{
  monitor_push(s, s->rnorm, s->gfnorm, s->gcnorm);
  if (s->cvg) {
    int reason = 0;
    int rc     = s->cvg(s->cvg_user, s->iteration, s->rnorm, &reason);
    if (rc) return pmh_set_error(PMH_ERR_ARG, "convergence test callback returned %d", rc);
    s->reason = reason;
  } else {
    PMH_CHK(converged_default(s));
  }
  return PMH_SUCCESS;
}

// ---- fused dual-space chain: emission by the vector kernels (pmh_op_s::emit_begin, emit_inline.h) ----------------------------
// the kernel about to be launched writes x (wx) and / or p (wp), one entry per thread: ea = it is filled and the EMIT variant must be launched, else nullptr
static const pmh_emit_args *emit_try(pmh_mpgp s, bool wx, bool wp, pmh_emit_args *ea)
{
  if (wx) s->cx[0] = false, s->x_applied = false;
  if (wp) s->cx[1] = false;
  if (s->csr || s->epi_ok != 1 || s->o.distributed || s->A->emit_begin(wx ? s->x : nullptr, wp ? s->work[4] : nullptr, ea) != PMH_SUCCESS) {
    if (wx) s->A->emit_invalidate();
    return nullptr;
  }
  if (wx) s->cx[0] = true;
  if (wp) s->cx[1] = true;
  return ea;
}

// The last step of a reduction whose block partials a kernel left in the pinned host copy, taken by the host after its wait: lane l of a wave of 64 adds its
// entries l, l + 64, ... in that order, then the butterflies of pmh_wave_all (emit_inline.h) -- the order in which a device consumer adds the same row
// (pmh_sum_block_partials), so both see the same number.
static double host_sum_row(const double *row, int nb, int op)
{
  double v[64];
  for (int l = 0; l < 64; l++) {
    double acc = (op == PMH_RED_SUM) ? 0.0 : INFINITY;
    for (int u = 0; u < 8; u++) {
      const double p = (l + 64 * u < nb) ? row[l + 64 * u] : ((op == PMH_RED_SUM) ? 0.0 : INFINITY);
      acc            = (op == PMH_RED_SUM) ? acc + p : fmin(acc, p);
    }
    v[l] = acc;
  }
  auto comb = [&](double a, double b) { return (op == PMH_RED_SUM) ? a + b : fmin(a, b); };
  double t[64];
  for (int l = 0; l < 64; l++) t[l] = comb(v[l], v[l ^ 1]);
  for (int l = 0; l < 64; l++) v[l] = comb(t[l], t[l ^ 2]);
  for (int l = 0; l < 64; l++) t[l] = comb(v[l], v[(l & ~7) | (7 - (l & 7))]);
  for (int l = 0; l < 64; l++) v[l] = comb(t[l], t[(l & ~15) | (15 - (l & 15))]);
  return comb(comb(v[0], v[16]), comb(v[32], v[48]));
}
// ---- owed_sums: the rows, ops and slots of the two groups, SPLIT first --------------------------------------------------------------------------------------
static const int OWED_OPS[7]   = {PMH_RED_SUM, PMH_RED_SUM, PMH_RED_SUM, PMH_RED_SUM, PMH_RED_SUM, PMH_RED_SUM, PMH_RED_MIN};
static const int OWED_SLOTS[7] = {S_APGF, S_GP2, S_GC2, S_GF2, S_PAP, S_GP, S_FEAS};
static const int OWED_P1_ROW   = 4; // the P1 rows as the operator's last kernel leaves them, behind a gradient split that may still wait

int owed_sums::finalize(pmh_ctx ctx, int group, int row, int nb, const int *halt, int *post)
{
  const int first = group == SPLIT ? 0 : OWED_P1_ROW, K = group == SPLIT ? 4 : 3;
  return pmh_finalize_partials(ctx, ctx->d_partials + (size_t)row * ctx->partials_cap, ctx->partials_cap, nb, K, OWED_OPS + first, OWED_SLOTS[first], halt, post);
}

int owed_sums::settle(pmh_ctx ctx, int groups, bool host_too, const int *halt, int *post)
{
  auto due = [&](int group, const rows &r) { return (groups & group) && (r.owed == DEVICE || (host_too && r.owed == HOST)); };
  const bool ds = due(SPLIT, split), dp = due(P1, p1);
  const int  nbs = split.nb, nbp = p1.nb;
  if (ds) split = rows();
  if (dp) p1 = rows();
  if (ds && dp && nbs == nbp && !ctx->dist_scalars && !halt && !post) return pmh_finalize_partials_slots(ctx, ctx->d_partials, ctx->partials_cap, nbs, 7, OWED_OPS, OWED_SLOTS);
  if (ds) PMH_CHK(finalize(ctx, SPLIT, 0, nbs, halt, post));
  if (dp) PMH_CHK(finalize(ctx, P1, OWED_P1_ROW, nbp));
  return PMH_SUCCESS;
}

void owed_sums::host_sums(pmh_ctx ctx)
{
  for (int k = 0; k < 7; k++) {
    const rows &r = k < OWED_P1_ROW ? split : p1;
    if (r.owed == HOST) ctx->h_scal[OWED_SLOTS[k]] = host_sum_row(ctx->h_partials + (size_t)k * ctx->partials_cap, r.nb, OWED_OPS[k]);
  }
  if (split.owed == HOST) split = rows();
  if (p1.owed == HOST) p1 = rows();
}

// the objective's one sum (k_obj_from_grad) -> S_TMP
static int finalize_obj(pmh_ctx ctx, int nb) { return pmh_finalize_partials(ctx, ctx->d_partials, ctx->partials_cap, nb, 1, OWED_OPS, S_TMP); }

// the solver's vectors as the phase launchers take them: work[1, 3, 4, 5] = gf, g, p, Ap (mpgp.c:6-17)
static phase_vecs vecs_of(pmh_mpgp s) { return phase_vecs{s->x, s->work[3], s->work[4], s->work[5], s->work[1], s->lb, s->ub, s->o.astol}; }

// a split, step or norms kernel has just left rows 0..3: the tile variant to the host, the plain one to its finalising launch, enqueued here
static int note_split(pmh_mpgp s, bool tile, const int *halt = nullptr, int *post = nullptr)
{
  s->owed.note(owed_sums::SPLIT, tile ? owed_sums::HOST : owed_sums::DEVICE, tile ? emit_blocks(s->n) : vec_blocks(s->n));
  return s->owed.settle(s->ctx, owed_sums::SPLIT, false, halt, post);
}

// --------------------------------------------------------------------------------------------------------------------
// unfused driver: QPSSolve_MPGP mpgp.c:438-650 call by call
// --------------------------------------------------------------------------------------------------------------------
static double *exp_direction(pmh_mpgp s)
{
  switch (s->o.exptype) { // mpgp.c:384-414
  case PMH_EXP_STD: return s->work[6];
  case PMH_EXP_GF: return s->work[1];
  case PMH_EXP_G: return s->work[3];
  case PMH_EXP_GFGR: return s->work[1];
  case PMH_EXP_GGR: return s->work[3];
  default: return s->work[1]; // projcg fallback vectors
  }
}
// the vector its length is measured by: the direction, but gr where the direction is gf or g with gr in its name
static double *exp_lengthvec(pmh_mpgp s) { return (s->o.exptype == PMH_EXP_GFGR || s->o.exptype == PMH_EXP_GGR) ? s->work[6] : exp_direction(s); }

// MPGPGrads mpgp.c:198-223
static int u_grads(pmh_mpgp s, const double *x, const double *g)
{
  PMH_CHK(pmh_qpc_box_grads(s->ctx, s->n, x, g, s->lb, s->ub, s->o.astol, s->work[1], s->work[2]));
  PMH_CHK(pmh_qpc_box_gradreduced(s->ctx, s->n, x, s->work[1], s->lb, s->ub, s->alpha, s->work[6]));
  return pmh_vec_waxpy(s->ctx, s->n, s->work[0], 1.0, s->work[1], s->work[2]);
}

// MPGPExpansionLength mpgp.c:233-287
static int u_expansion_length(pmh_mpgp s, double *xold, double *explengthvecold)
{
  pmh_ctx ctx = s->ctx;
  int     n   = s->n;
  double *lv  = exp_lengthvec(s), dots[2];
  switch (s->o.explengthtype) {
  case PMH_EXPLEN_FIXED: break;
  case PMH_EXPLEN_OPT:
    PMH_CHK(s->A->mult(lv, s->work[5]));
    s->nmv++;
    PMH_CHK(pmh_vec_dot(ctx, n, lv, s->work[3], &dots[0]));
    PMH_CHK(pmh_vec_dot(ctx, n, lv, s->work[5], &dots[1]));
    if (dots[1] == .0 && s->o.resetalpha) s->alpha = s->alpha / s->maxeig;
    else s->alpha = s->alpha_user * (dots[0] / dots[1]);
    break;
  case PMH_EXPLEN_OPTAPPROX:
    if (s->work[3] != lv) {
      PMH_CHK(pmh_vec_dot(ctx, n, lv, s->work[3], &dots[0]));
      PMH_CHK(pmh_vec_dot(ctx, n, lv, lv, &dots[1]));
      s->alpha = s->alpha_user * (dots[0] / dots[1]);
    } else {
      s->alpha = s->alpha_user;
    }
    s->alpha = s->alpha / s->maxeig;
    break;
  case PMH_EXPLEN_BB:
    PMH_CHK(pmh_vec_aypx(ctx, n, explengthvecold, -1.0, lv));
    PMH_CHK(pmh_vec_aypx(ctx, n, xold, -1.0, s->x));
    PMH_CHK(pmh_vec_dot(ctx, n, explengthvecold, explengthvecold, &dots[0]));
    PMH_CHK(pmh_vec_dot(ctx, n, explengthvecold, xold, &dots[1]));
    if (dots[1] == .0 && s->o.resetalpha) s->alpha = s->alpha / s->maxeig;
    else s->alpha = s->alpha_user * (dots[0] / dots[1]);
    break;
  }
  return PMH_SUCCESS;
}

// MPGPExpansion_Std mpgp.c:299-323
static int u_expansion_std(pmh_mpgp s, double afeas, double *xold, double *explengthvecold)
{
  pmh_ctx ctx = s->ctx;
  int     n   = s->n;
  PMH_CHK(pmh_vec_axpy(ctx, n, s->x, -afeas, s->work[4]));
  PMH_CHK(pmh_vec_axpy(ctx, n, s->work[3], -afeas, s->work[5]));
  PMH_CHK(u_grads(s, s->x, s->work[3]));
  PMH_CHK(u_expansion_length(s, xold, explengthvecold));
  return pmh_vec_axpy(ctx, n, s->x, -s->alpha, exp_direction(s));
}

static int u_objective_from_gradient(pmh_mpgp s, const double *x, const double *g, double *f)
{
  PMH_CHK(phase_obj(s->ctx, s->n, x, g, s->b));
  PMH_CHK(finalize_obj(s->ctx, vec_blocks(s->n)));
  double v;
  PMH_CHK(pmh_host_scalar(s->ctx, S_TMP, &v));
  *f = .5 * v;
  return PMH_SUCCESS;
}

static int solve_unfused(pmh_mpgp s)
{
  s->g_valid  = 0; // (this driver always forms its own gradient)
  s->x_applied = false, s->first_applied = 0;
  s->cx[0] = s->cx[1] = false;
  s->A->emit_invalidate();
  pmh_ctx ctx = s->ctx;
  int     n   = s->n;
  int     nw  = 7;
  if (s->o.fallback || s->o.fallback2) nw = (s->o.explengthtype != PMH_EXPLEN_BB) ? 9 : 10; // mpgp.c:366-376
  else if (s->o.explengthtype == PMH_EXPLEN_BB) nw = 9;
  for (int i = 0; i < nw; i++) PMH_CHK(ensure_work(s, i));
  double *gP = s->work[0], *gf = s->work[1], *gc = s->work[2], *g = s->work[3], *p = s->work[4], *Ap = s->work[5];
  double *gold = nullptr, *xold = nullptr, *explengthvecold = nullptr;
  if (s->o.explengthtype == PMH_EXPLEN_BB) { // mpgp.c:479-486
    explengthvecold = s->work[7];
    xold            = s->work[8];
    if (s->o.fallback || s->o.fallback2) gold = s->work[9];
  } else if (s->o.fallback || s->o.fallback2) {
    xold = s->work[7];
    gold = s->work[8];
  }
  const double gamma2 = s->o.gamma * s->o.gamma;
  double       acg, bcg, afeas, pAp, gcTgc, gfTgf, f, fold;
  int          nmv = 0, ncg = 0, nprop = 0, nexp = 0, nfinc = 0, nfall = 0;
  int          fallback = s->fallback_state;
  double      *x = s->x;

  PMH_CHK(pmh_qpc_box_project(ctx, n, x, s->lb, s->ub, x)); // mpgp.c:497
  PMH_CHK(s->A->mult(x, g));
  nmv++;
  PMH_CHK(pmh_vec_axpy(ctx, n, g, -1.0, s->b));
  PMH_CHK(u_grads(s, x, g));
  PMH_CHK(pmh_vec_copy(ctx, n, gf, p));
  s->step      = ' ';
  s->iteration = 0;
  while (1) {
    PMH_CHK(phase_three_norms(ctx, n, gP, gc, gf));
    PMH_CHK(note_split(s, false));
    PMH_CHK(pmh_sync(ctx));
    s->rnorm  = sqrt(ctx->h_scal[S_GP2]);
    gcTgc     = ctx->h_scal[S_GC2];
    gfTgf     = ctx->h_scal[S_GF2];
    s->gfnorm = sqrt(gfTgf);
    s->gcnorm = sqrt(gcTgc);
    PMH_CHK(test_convergence(s));
    if (s->reason != PMH_CONVERGED_ITERATING) break;

    if (gcTgc <= gamma2 * gfTgf) {
      PMH_CHK(s->A->mult(p, Ap));
      nmv++;
      PMH_CHK(pmh_vec_dot(ctx, n, p, Ap, &pAp));
      PMH_CHK(pmh_vec_dot(ctx, n, g, p, &acg));
      acg = acg / pAp;
      PMH_CHK(pmh_qpc_box_feas(ctx, n, x, p, s->lb, s->ub, &afeas));
      if (acg <= afeas) {
        ncg++;
        s->step = 'c';
        PMH_CHK(pmh_vec_axpy(ctx, n, x, -acg, p));
        PMH_CHK(pmh_vec_axpy(ctx, n, g, -acg, Ap));
        PMH_CHK(u_grads(s, x, g));
        PMH_CHK(pmh_vec_dot(ctx, n, Ap, gf, &bcg));
        bcg = bcg / pAp;
        PMH_CHK(pmh_vec_aypx(ctx, n, p, -bcg, gf));
      } else {
        nexp++;
        s->step = 'e';
        if (s->o.explengthtype == PMH_EXPLEN_BB || fallback || s->o.fallback2) {
          PMH_CHK(pmh_vec_copy(ctx, n, x, xold));
          if (s->o.explengthtype == PMH_EXPLEN_BB) PMH_CHK(pmh_vec_copy(ctx, n, exp_lengthvec(s), explengthvecold));
        }
        if (s->o.exptype == PMH_EXP_PROJCG) PMH_CHK(pmh_vec_axpy(ctx, n, x, -acg, p)); // MPGPExpansion_ProjCG mpgp.c:335-349
        else PMH_CHK(u_expansion_std(s, afeas, xold, explengthvecold));
        if (s->expproject) PMH_CHK(pmh_qpc_box_project(ctx, n, x, s->lb, s->ub, x));
        if (fallback || s->o.fallback2) PMH_CHK(pmh_vec_copy(ctx, n, g, gold));
        PMH_CHK(s->A->mult(x, g));
        nmv++;
        PMH_CHK(pmh_vec_axpy(ctx, n, g, -1.0, s->b));
        if (fallback || s->o.fallback2) {
          PMH_CHK(u_objective_from_gradient(s, xold, gold, &fold));
          PMH_CHK(u_objective_from_gradient(s, x, g, &f));
          if (f > fold) {
            nfinc++;
            if (s->o.fallback2) {
              PMH_CHK(u_grads(s, x, g));
              PMH_CHK(pmh_vec_dot(ctx, n, gc, gc, &gcTgc));
              PMH_CHK(pmh_vec_dot(ctx, n, gf, gf, &gfTgf));
              fallback = (gcTgc <= gamma2 * gfTgf) ? 0 : 1;
            }
            if (fallback) {
              nfall++;
              s->step = 'f';
              PMH_CHK(pmh_vec_copy(ctx, n, xold, x));
              PMH_CHK(pmh_vec_copy(ctx, n, gold, g));
              if (s->o.fallback2) PMH_CHK(u_grads(s, xold, gold));
              PMH_CHK(u_expansion_std(s, afeas, xold, explengthvecold));
              PMH_CHK(pmh_qpc_box_project(ctx, n, x, s->lb, s->ub, x));
              PMH_CHK(s->A->mult(x, g));
              nmv++;
              PMH_CHK(pmh_vec_axpy(ctx, n, g, -1.0, s->b));
            }
          }
        }
        PMH_CHK(u_grads(s, x, g));
        PMH_CHK(pmh_vec_copy(ctx, n, gf, p));
      }
    } else {
      nprop++;
      s->step = 'p';
      PMH_CHK(pmh_vec_copy(ctx, n, gc, p));
      PMH_CHK(s->A->mult(p, Ap));
      nmv++;
      PMH_CHK(pmh_vec_dot(ctx, n, p, Ap, &pAp));
      PMH_CHK(pmh_vec_dot(ctx, n, g, p, &acg));
      acg = acg / pAp;
      PMH_CHK(pmh_vec_axpy(ctx, n, x, -acg, p));
      PMH_CHK(pmh_vec_axpy(ctx, n, g, -acg, Ap));
      PMH_CHK(u_grads(s, x, g));
      PMH_CHK(pmh_vec_copy(ctx, n, gf, p));
    }
    s->iteration++;
  }
  s->fallback_state = fallback;
  s->ncg += ncg, s->nexp += nexp, s->nmv += nmv, s->nprop += nprop, s->nfinc += nfinc, s->nfall += nfall;
  return PMH_SUCCESS;
}

// --------------------------------------------------------------------------------------------------------------------
// fused driver (std expansion, fixed step length, no fallback)
// --------------------------------------------------------------------------------------------------------------------
// P1: Ap = A p and the three reductions into d_scal/h_scal[S_PAP..S_FEAS]
static int f_apply_p1(pmh_mpgp s, const int *halt = nullptr, bool p_fresh = false)
{
  double *g = s->work[3], *p = s->work[4], *Ap = s->work[5];
  s->x_applied = false; // the operator's last application is to p from here on
  if (s->csr) {
    pmh_spmv_epi e;
    memset(&e, 0, sizeof(e));
    e.kind = PMH_EPI_MPGP, e.g = g, e.xx = s->x, e.lb = s->lb, e.ub = s->ub, e.scal_base = S_PAP, e.halt = halt;
    return pmh_csr_spmv_launch(s->csr, p, Ap, e);
  }
  if (halt) return pmh_set_error(PMH_ERR_STATE, "speculative chain needs a CSR operator");
  pmh_ctx   ctx = s->ctx;
  const int nb  = vec_blocks(s->n);
  // the three reductions inside the operator's last kernel (rows 4..6 of the partials: rows 0..3 may still hold a gradient split that waits for its finalising
  // launch)
  if (s->epi_ok) {
    pmh_vec_epi e;
    memset(&e, 0, sizeof(e));
    e.kind = PMH_VEPI_P1, e.g = g, e.xx = s->x, e.lb = s->lb, e.ub = s->ub, e.partials = s->ctx->d_partials, e.ld = s->ctx->partials_cap, e.prow = 4;
    e.p_fresh = p_fresh, e.spec_alpha = s->alpha, e.astol = s->o.astol; // (operators that pair their passes: svm.hip)
    int hosted = 0;
    // (the fused dual-space chain: G0 p left behind by the kernel that wrote p; the three sums' block partials go to the pinned host copy)
    e.in_slot = s->cx[1] ? 2 : 0, e.hosted = s->ctx->dist_scalars ? nullptr : &hosted;
    const int rc = s->A->mult_epi(p, Ap, e);
    if (rc != PMH_EPI_UNSUPPORTED) {
      PMH_CHK(rc);
      s->epi_ok = 1;
      // hosted: the host adds these three, and a gradient split that waits for a launch gets its own (one that waits for the host goes on waiting); else with
      // such a split (Ap'gf, |gP|^2, |gc|^2, |gf|^2) and (p'Ap, g'p, afeas) in ONE finalising launch
      s->owed.note(owed_sums::P1, hosted ? owed_sums::HOST : owed_sums::DEVICE, hosted ? hosted : nb);
      return s->owed.settle(ctx, owed_sums::SPLIT | owed_sums::P1);
    }
    s->epi_ok = 0;
  }
  // a split that still waits for its launch sits in the rows k_p1_dots is about to overwrite
  PMH_CHK(s->owed.settle(ctx, owed_sums::SPLIT));
  PMH_CHK(s->A->mult(p, Ap));
  PMH_CHK(phase_p1_dots(ctx, s->n, vecs_of(s)));
  return owed_sums::finalize(ctx, owed_sums::P1, 0, nb);
}

// g = A x - b (mpgp.c:500-502, :578-580)
static int f_gradient(pmh_mpgp s, bool same_input = false, int *replayed = nullptr)
{
  double *g = s->work[3];
  if (s->csr) {
    pmh_spmv_epi e;
    memset(&e, 0, sizeof(e));
    e.kind = PMH_EPI_SUB, e.y1 = s->b;
    return pmh_csr_spmv_launch(s->csr, s->x, g, e);
  }
  PMH_CHK(same_input ? s->A->mult_same_input(s->x, g, replayed) : s->A->mult(s->x, g));
  return pmh_vec_axpy(s->ctx, s->n, g, -1.0, s->b);
}

// g = A x - b, the gradient split with p = gf and the partials of its norms (mpgp.c:500-507, :578-580 + :612-615): inside the operator's last kernel where it
// offers that (defer_finalize: the finalising launch then waits for the next P1, owed_sums), else as three launches + the finalising one
// same_input: x still holds what the operator was last applied to (pmh_vec_epi::same_input); *replayed = 1 where the operator took that word
static int f_gradient_split(pmh_mpgp s, bool defer_finalize, bool x_from_spec = false, bool same_input = false, int *replayed = nullptr)
{
  pmh_ctx ctx = s->ctx;
  double *gf = s->work[1], *g = s->work[3], *p = s->work[4];
  s->x_applied = true; // whichever form follows applies the operator to x, last of all
  if (s->epi_ok && !s->csr) {
    pmh_vec_epi e;
    memset(&e, 0, sizeof(e));
    e.kind = PMH_VEPI_GRAD_SPLIT, e.b = s->b, e.lb = s->lb, e.ub = s->ub, e.astol = s->o.astol, e.gf = gf, e.p = p, e.partials = ctx->d_partials, e.ld = ctx->partials_cap, e.prow = 0;
    e.x_from_spec = x_from_spec, e.x_out = s->x, e.same_input = same_input;
    int hosted = 0, p_emitted = 0;
    e.in_slot = s->cx[0] ? 1 : 0, e.hosted = ctx->dist_scalars ? nullptr : &hosted, e.emitted_p = &p_emitted, e.replayed = replayed;
    const int rc = s->A->mult_epi(s->x, g, e);
    if (rc != PMH_EPI_UNSUPPORTED) {
      PMH_CHK(rc);
      s->epi_ok = 1;
      s->cx[1]  = p_emitted != 0; // p = gf was written by the operator's last kernel
      s->owed.note(owed_sums::SPLIT, hosted ? owed_sums::HOST : owed_sums::DEVICE, hosted ? hosted : vec_blocks(s->n));
      if (hosted || (defer_finalize && !ctx->dist_scalars)) return PMH_SUCCESS;
      return s->owed.settle(ctx, owed_sums::SPLIT);
    }
    s->epi_ok = 0;
  }
  if (x_from_spec) return pmh_set_error(PMH_ERR_STATE, "pmh_mpgp: the operator prepared an expansion step and then refused the gradient");
  PMH_CHK(f_gradient(s, same_input, replayed));
  s->cx[1] = false;
  PMH_CHK(phase_split(ctx, s->n, vecs_of(s), nullptr));
  return note_split(s, false);
}

// ---- the steps of the fused driver: QPSSolve_MPGP (mpgp.c:438-650) cut where the reference's loop branches ------------------------------------------------
static const int SPEC_BATCH = 16; // the longest batch of the device-side CG chain, and the room of its ring

struct fused_state {
  bool spec = false; // P1 for the current p already enqueued
  // length of the next speculative batch: a batch that ran to its end doubles it, one that halted early cuts it to what it ran (an expansion-heavy stretch
  // would otherwise enqueue 16 x 4 no-op launches behind every expansion step: ~0.1 ms each time); 0 = the host takes the next step.  The iterates do not
  // depend on it: the device chain takes exactly the steps the host would.
  int    spec_len         = SPEC_BATCH;
  bool   p_fresh          = false; // p is the gf of the last gradient split, untouched (told to operators that pair their passes)
  double prev_margin      = 0.0;   // cvg_margin of the previous test (f_speculate_next)
  bool   check_projection = false; // the first gradient took the caller's word: the projection's word is read after the first wait (f_host_test)
  int    nmv = 0, ncg = 0, nexp = 0, nprop = 0;
};

// the projection of the start (mpgp.c:497) and the first gradient with its split and p = gf (:500-507), carried or formed
static int f_first_gradient(pmh_mpgp s, fused_state &st)
{
  pmh_ctx   ctx = s->ctx;
  const int n   = s->n;
  s->cx[0] = s->cx[1] = false; // x and p come from outside
  s->owed.clear();
  // The caller's word (pmh_mpgp_set_first_operand_applied) that x is the vector the operator was last applied to: the operator keeps what it remembers of that
  // application, and the first gradient below passes the word on.  The projection rewrites a feasible x with the bits it had -- but the x an expansion step
  // leaves (x - afeas p - alpha gr, no re-projection) may lie below a bound by a rounding error, and then the projection does change it.  So the projection
  // leaves a word for the host where it changed an entry, read after the first wait (f_host_test, no wait of its own): the gradient is then taken again, in
  // full.  (Not with row-distributed vectors: that word would be each rank's own.)
  const bool first_same = s->first_applied != 0 && !s->g_valid && !s->o.distributed;
  s->first_applied = 0, s->x_applied = false;
  s->A->emit_invalidate(first_same);
  if (first_same) PMH_CHK(pmh_qpc_box_project_flag(ctx, n, s->x, s->lb, s->ub, s->x, PMH_SLOT_PROJ_CHANGED));
  else PMH_CHK(pmh_qpc_box_project(ctx, n, s->x, s->lb, s->ub, s->x)); // mpgp.c:497
  // asked once: a refusal (PMH_EPI_UNSUPPORTED) clears it.  (Row-distributed vectors: the operator's partials are finalised at once and completed across the
  // ranks, pmh_finalize_partials)
  if (s->epi_ok < 0) s->epi_ok = (s->csr || !pmh_knobs().vec_epi) ? 0 : 1;
  if (s->g_valid) { // the caller carried g = A x - b over from the previous solve (pmh_smalxe_set_reuse_products): the split, p = gf and the norms only
    // (the operator's own gradient split does not run: whatever pairing state an operator keeps from the previous solve must not be matched with this p --
    // p_fresh stays false, the first product of the solve is then a lone application)
    s->g_valid = 0;
    pmh_emit_args        ea;
    const pmh_emit_args *e = emit_try(s, false, true, &ea);
    PMH_CHK(phase_split(ctx, n, vecs_of(s), e));
    return note_split(s, e);
  }
  int replayed = 0;
  PMH_CHK(f_gradient_split(s, false, false, first_same, &replayed)); // :500-507 (the host reads the norms before any P1: finalised at once)
  st.check_projection = first_same && replayed != 0;                  // the operator did take the caller's word
  st.nmv++, st.p_fresh = true;
  return PMH_SUCCESS;
}

// the device-side CG chain needs the default convergence test (its constants go to the kernels) and a CSR operator: sa->ctl stays null where this solve has none
static int f_spec_setup(pmh_mpgp s, double gamma2, pmh_spec_args *sa)
{
  pmh_ctx ctx = s->ctx;
  if (!(s->csr && !s->cvg && !s->o.distributed && pmh_knobs().mpgp_spec)) return PMH_SUCCESS;
  if (!s->d_ctl) {
    PMH_CHK(pmh_malloc(ctx, sizeof(int) * CTL_NWORDS, (void **)&s->d_ctl));
    PMH_CHK(pmh_malloc(ctx, sizeof(double) * 3 * SPEC_BATCH, (void **)&s->d_ring));
    PMH_HIP(hipHostMalloc((void **)&s->h_ctl, sizeof(int) * CTL_NWORDS, hipHostMallocMapped));
    PMH_HIP(hipHostMalloc((void **)&s->h_ring, sizeof(double) * 3 * SPEC_BATCH, hipHostMallocMapped));
  }
  PMH_CHK(converged_default_setup(s));
  sa->ctl = s->d_ctl, sa->ring = s->d_ring, sa->ring_cap = SPEC_BATCH, sa->max_it = s->o.max_it;
  sa->ttol = s->ttol, sa->divtol_rhs = s->o.divtol * s->norm_rhs_div, sa->gamma2 = gamma2;
  return PMH_SUCCESS;
}

// a batch of CG steps decided on the device (the SPEC variant of k_step_update: the test of mpgp.c:531, :535 and :547 from the device scalars): no host round trip between
// them.  *halted = false: the whole batch were CG steps
static int f_spec_batch(pmh_mpgp s, fused_state &st, const pmh_spec_args &sa, bool *halted)
{
  pmh_ctx          ctx = s->ctx;
  const int        n = s->n, nbatch = st.spec_len;
  const phase_vecs v    = vecs_of(s);
  int             *halt = s->d_ctl + CTL_HALT;
  s->x_applied          = false;
  s->h_ctl[CTL_HALT] = 0, s->h_ctl[CTL_ITER] = s->iteration, s->h_ctl[CTL_NCG] = 0, s->h_ctl[CTL_BASE] = s->iteration;
  PMH_HIP(hipMemcpyAsync(s->d_ctl, s->h_ctl, sizeof(int) * CTL_NWORDS, hipMemcpyHostToDevice, ctx->stream));
  for (int j = 0; j < nbatch; j++) {
    PMH_CHK(phase_step(ctx, n, v, false, &sa, nullptr, 0.0, 0));
    PMH_CHK(note_split(s, false, halt, s->d_ctl + CTL_ITER));
    PMH_CHK(phase_dir(ctx, n, v, halt, nullptr, 0, 0.0));
    PMH_CHK(f_apply_p1(s, halt));
  }
  PMH_HIP(hipMemcpyAsync(s->h_ctl, s->d_ctl, sizeof(int) * CTL_NWORDS, hipMemcpyDeviceToHost, ctx->stream));
  PMH_HIP(hipMemcpyAsync(s->h_ring, s->d_ring, sizeof(double) * 3 * SPEC_BATCH, hipMemcpyDeviceToHost, ctx->stream));
  PMH_CHK(pmh_sync(ctx));
  const int ndev = s->h_ctl[CTL_ITER] - s->iteration;
  for (int j = 0; j < ndev; j++) {
    monitor_push(s, sqrt(s->h_ring[3 * j]), sqrt(s->h_ring[3 * j + 1]), sqrt(s->h_ring[3 * j + 2])); // QPSMonitorDefault_MPGP line of iteration s->iteration + j
    s->step = 'c';
  }
  s->iteration += ndev, st.ncg += ndev, st.nmv += ndev;
  // 0 after a batch that took no step: the host path decides when speculation resumes
  st.spec_len = (ndev >= nbatch) ? std::min(SPEC_BATCH, 2 * nbatch) : ndev;
  *halted     = s->h_ctl[CTL_HALT] != 0;
  return PMH_SUCCESS;
}

// the host's test: the norms of the split (mpgp.c:514-521), the monitor (:524-528) and the convergence test (:531) -> s->reason
static int f_host_test(pmh_mpgp s, fused_state &st, double *gcTgc, double *gfTgf)
{
  pmh_ctx ctx = s->ctx;
  if (s->pre_test) PMH_CHK(s->pre_test(s->pre_test_user));
  PMH_CHK(pmh_sync(ctx));
  if (st.check_projection) {
    st.check_projection = false;
    // The projection did change an entry: what the operator kept belongs to the vector as it was before.  Everything the first gradient wrote (g, gf, p, the
    // partial sums, the emitted sums) is written again by the full application to the projected x -- the launches a solve without the caller's word makes
    // (and its note replaces what the first gradient left to the host).  Several ranks: x is replicated bit for bit and every rank ran the same projection on
    // it, so every rank reads the same word here and all of them enter the full application's all-reduce, or none does
    if (ctx->h_scal[PMH_SLOT_PROJ_CHANGED] != 0.0) {
      pmh_knobs().chain_replays_redone++;
      s->A->emit_invalidate();
      PMH_CHK(f_gradient_split(s, false));
      PMH_CHK(pmh_sync(ctx));
    }
  }
  s->owed.host_sums(ctx);
  s->rnorm  = sqrt(ctx->h_scal[S_GP2]);
  *gcTgc    = ctx->h_scal[S_GC2];
  *gfTgf    = ctx->h_scal[S_GF2];
  s->gfnorm = sqrt(*gfTgf);
  s->gcnorm = sqrt(*gcTgc);
  return test_convergence(s);
}

// CG step (mpgp.c:547-560)
static int f_cg_step(pmh_mpgp s, fused_state &st, double acg, double pAp)
{
  pmh_ctx          ctx = s->ctx;
  const int        n   = s->n;
  const phase_vecs v   = vecs_of(s);
  st.ncg++, s->step = 'c';
  st.spec_len = std::max(st.spec_len, 1); // a CG step taken by the host: the next ones may well be CG steps too
  pmh_emit_args ea;
  // x -= acg p with the segment sums of G0 x left behind; acg as the host has it; the four sums' block partials go to the pinned host copy
  const pmh_emit_args *e = emit_try(s, true, false, &ea);
  PMH_CHK(phase_step(ctx, n, v, false, nullptr, e, acg, 0));
  PMH_CHK(note_split(s, e));
  const pmh_emit_args *ep = e ? emit_try(s, false, true, &ea) : nullptr;
  if (!ep) { // the plain direction kernel takes Ap'gf from d_scal: a step that left its sums to the host has them finalised on the device after all
    PMH_CHK(s->owed.settle(ctx, owed_sums::SPLIT, true));
    s->cx[1] = false;
  }
  PMH_CHK(phase_dir(ctx, n, v, nullptr, ep, emit_blocks(n), pAp));
  st.p_fresh = false;
  return PMH_SUCCESS;
}

// expansion step (mpgp.c:561-616), std direction + fixed length => no re-projection (:388), with the gradient at the new x (:578-580) and its split (:612-615)
static int f_expansion_step(pmh_mpgp s, fused_state &st, double afeas)
{
  st.nexp++, s->step = 'e';
  // the operator's P1 pass already formed k_expansion_std's iterate (svm.hip): it hands it over with the gradient
  const bool prepared = s->epi_ok == 1 && s->A->spec_expansion_ready();
  if (!prepared) {
    pmh_emit_args ea;
    PMH_CHK(phase_expansion(s->ctx, s->n, vecs_of(s), afeas, s->alpha, emit_try(s, true, false, &ea)));
  } else {
    s->cx[0] = false;
    s->A->emit_invalidate();
  }
  PMH_CHK(f_gradient_split(s, true, prepared)); // the speculative P1 (f_speculate_next) finalises both groups of partial sums
  st.nmv++, st.p_fresh = true;
  return PMH_SUCCESS;
}

// proportioning step (mpgp.c:617-639)
static int f_proportioning_step(pmh_mpgp s, fused_state &st)
{
  pmh_ctx          ctx = s->ctx;
  const int        n   = s->n;
  const phase_vecs v   = vecs_of(s);
  st.nprop++, s->step = 'p';
  st.spec = st.p_fresh = false; // a speculative P1 (if any) used the wrong direction; it is simply not counted
  pmh_emit_args ea;
  PMH_CHK(phase_prop_dir(ctx, n, v, emit_try(s, false, true, &ea)));
  PMH_CHK(f_apply_p1(s));
  st.nmv++;
  // the product left its sums to the host: the step forms acg from the P1 block partials itself (no host wait in between).  Otherwise the step reads acg from
  // d_scal: P1 rows that were left to the host are finalised on the device after all
  const pmh_emit_args *e = s->owed.p1.owed == owed_sums::HOST ? emit_try(s, true, true, &ea) : nullptr;
  if (!e) {
    PMH_CHK(s->owed.settle(ctx, owed_sums::P1, true));
    s->cx[0] = s->cx[1] = false;
  }
  PMH_CHK(phase_step(ctx, n, v, true, nullptr, e, 0.0, s->owed.p1.nb));
  return note_split(s, e);
}

// Speculation: whatever the next step type, unless it is a proportioning step it starts with Ap = A p -- enqueued before the host has seen this step's norms,
// so that the round trip costs nothing.  If the NEXT test ends the solve that product is wasted (0.35 ms for configs[2] against the ~30 us of an exposed round
// trip): the test reports how far the norm is above its threshold (cvg_margin), and with the last step's reduction the driver skips the speculation when the
// next norm is likely to pass (SMALXE's early outer iterations end their inner solves after 2-3 steps: 8 of 63 products in the driver's 20-step window were
// such orphans).  Nothing numerical depends on it: the product is then enqueued after the test, by the `!st.spec` branch of the loop.
static int f_speculate_next(pmh_mpgp s, fused_state &st)
{
  bool         orphan_risk = false;
  const double m           = s->cvg_margin;
  if (m > 0.0) {
    const double red = (st.prev_margin > 0.0 && m < st.prev_margin) ? m / st.prev_margin : 1.0;
    orphan_risk      = (m < 3.0) || (m * red < 2.0);
  }
  st.prev_margin = m;
  if (orphan_risk) {
    st.spec = false;
    return s->owed.settle(s->ctx, owed_sums::SPLIT); // a gradient split that left its sums for the product's finalising launch: the host reads the norms next
  }
  if (s->pre_p1) PMH_CHK(s->pre_p1(s->pre_p1_user));
  PMH_CHK(f_apply_p1(s, nullptr, st.p_fresh));
  st.spec = true;
  return PMH_SUCCESS;
}

static int solve_fused(pmh_mpgp s)
{
  pmh_ctx ctx = s->ctx;
  for (int i : {1, 3, 4, 5}) PMH_CHK(ensure_work(s, i));
  const double gamma2 = s->o.gamma * s->o.gamma;
  fused_state  st;
  PMH_CHK(f_first_gradient(s, st)); // mpgp.c:497-507
  s->step = ' ', s->iteration = 0;
  pmh_spec_args sa = {};
  PMH_CHK(f_spec_setup(s, gamma2, &sa));
  while (1) {
    if (sa.ctl && st.spec && st.spec_len > 0) {
      bool halted;
      PMH_CHK(f_spec_batch(s, st, sa, &halted));
      if (!halted) continue; // whole batch were CG steps
    }
    double gcTgc, gfTgf;
    PMH_CHK(f_host_test(s, st, &gcTgc, &gfTgf)); // mpgp.c:514-531
    if (s->reason != PMH_CONVERGED_ITERATING) break;

    if (gcTgc <= gamma2 * gfTgf) { // proportional (mpgp.c:535)
      if (!st.spec) {
        PMH_CHK(f_apply_p1(s, nullptr, st.p_fresh));
        PMH_CHK(pmh_sync(ctx));
        s->owed.host_sums(ctx);
      }
      st.spec = false;
      st.nmv++;
      const double pAp = ctx->h_scal[S_PAP], acg = ctx->h_scal[S_GP] / pAp, afeas = ctx->h_scal[S_FEAS]; // mpgp.c:541-546
      if (acg <= afeas) PMH_CHK(f_cg_step(s, st, acg, pAp)); // mpgp.c:547-560
      else PMH_CHK(f_expansion_step(s, st, afeas));          // mpgp.c:561-616
    } else {
      PMH_CHK(f_proportioning_step(s, st)); // mpgp.c:617-639
    }
    PMH_CHK(f_speculate_next(s, st));
    s->iteration++;
  }
  s->ncg += st.ncg, s->nexp += st.nexp, s->nmv += st.nmv, s->nprop += st.nprop;
  return PMH_SUCCESS;
}

extern "C" int pmh_mpgp_solve(pmh_mpgp s)
{
  PMH_ARG(s);
  s->t_step.clear(), s->t_gp.clear(), s->t_gf.clear(), s->t_gc.clear(), s->t_alpha.clear();
  s->ctx->dist_scalars = s->o.distributed;
  int rc               = use_fused(s) ? solve_fused(s) : solve_unfused(s);
  s->ctx->dist_scalars = 0;
  return rc;
}

extern "C" int pmh_mpgp_get_tolerances(pmh_mpgp s, double *rtol, double *atol, double *divtol, int *max_it) // QPSGetTolerances
{
  PMH_ARG(s);
  if (rtol) *rtol = s->o.rtol;
  if (atol) *atol = s->o.atol;
  if (divtol) *divtol = s->o.divtol;
  if (max_it) *max_it = s->o.max_it;
  return PMH_SUCCESS;
}

extern "C" int pmh_mpgp_get_stats(pmh_mpgp s, pmh_mpgp_stats *st)
{
  PMH_ARG(s && st);
  memset(st, 0, sizeof(*st));
  st->iteration = s->iteration, st->reason = s->reason;
  st->rnorm = s->rnorm, st->gfnorm = s->gfnorm, st->gcnorm = s->gcnorm, st->alpha = s->alpha, st->maxeig = s->maxeig;
  st->nmv = s->nmv, st->ncg = s->ncg, st->nexp = s->nexp, st->nprop = s->nprop, st->nfinc = s->nfinc, st->nfall = s->nfall;
  st->norm_rhs = s->norm_rhs, st->ttol = s->ttol;
  st->current_step_type = s->step;
  return PMH_SUCCESS;
}

extern "C" int pmh_mpgp_get_trace(pmh_mpgp s, int cap, char *step, double *gp, double *gf, double *gc, double *alpha, int *len)
{
  PMH_ARG(s && len);
  int m = (int)s->t_step.size();
  *len  = m;
  if (m > cap) m = cap;
  for (int i = 0; i < m; i++) {
    if (step) step[i] = s->t_step[i];
    if (gp) gp[i] = s->t_gp[i];
    if (gf) gf[i] = s->t_gf[i];
    if (gc) gc[i] = s->t_gc[i];
    if (alpha) alpha[i] = s->t_alpha[i];
  }
  return PMH_SUCCESS;
}

// work[0..6] = gP, gf, gc, g, p, Ap, gr (mpgp.c:6-17).  The fused driver does not keep gP, gc, gr:
// they are recomputed here from the final x, g (MPGPGrads) so that callers see the reference's work vectors.
// internal (an injected convergence test says how close it is to ending the solve, see solve_fused's speculation)
int pmh_mpgp_set_convergence_margin(pmh_mpgp s, double margin)
{
  PMH_ARG(s);
  s->cvg_margin = margin;
  return PMH_SUCCESS;
}

// internal (smalxe.hip): see pmh_internal.h
int pmh_mpgp_x_applied(pmh_mpgp s) { return (s && s->x_applied) ? 1 : 0; }
int pmh_mpgp_set_first_operand_applied(pmh_mpgp s, int on)
{
  PMH_ARG(s);
  s->first_applied = (on && use_fused(s)) ? 1 : 0;
  return PMH_SUCCESS;
}

// internal (smalxe.hip): the next pmh_mpgp_solve may take work[3] as the gradient at its starting point (fused driver only; others ignore it)
int pmh_mpgp_set_gradient_valid(pmh_mpgp s, int valid, double **g)
{
  PMH_ARG(s);
  s->g_valid = (valid && use_fused(s) && s->work[3]) ? 1 : 0;
  if (g) *g = s->work[3];
  return PMH_SUCCESS;
}

extern "C" int pmh_mpgp_get_work(pmh_mpgp s, int idx, const double **dptr)
{
  PMH_ARG(s && dptr && idx >= 0 && idx < 10);
  if (use_fused(s) && (idx == 0 || idx == 2 || idx == 6)) {
    PMH_ARG(s->work[3]);
    PMH_CHK(ensure_work(s, 0));
    PMH_CHK(ensure_work(s, 2));
    PMH_CHK(ensure_work(s, 6));
    PMH_CHK(ensure_work(s, 1));
    PMH_CHK(u_grads(s, s->x, s->work[3]));
  }
  PMH_ARG(s->work[idx]);
  *dptr = s->work[idx];
  return PMH_SUCCESS;
}

// --------------------------------------------------------------------------------------------------------------------
// test entries (include/permon_hip.h): one phase kernel, or one reduction finisher, on the caller's data.  No solver calls them.
// --------------------------------------------------------------------------------------------------------------------
extern "C" int pmh_mpgp_test_host_sum_row(const double *row, int nb, int op, double *out)
{
  PMH_ARG(out && nb >= 0 && nb <= 512 && (row || !nb) && (op == PMH_RED_SUM || op == PMH_RED_MIN));
  *out = host_sum_row(row, nb, op);
  return PMH_SUCCESS;
}

__global__ __launch_bounds__(64) void k_test_block_sum(const double *__restrict__ row, int nb, double *__restrict__ out)
{
  out[threadIdx.x] = pmh_sum_block_partials(row, nb);
}

extern "C" int pmh_mpgp_test_block_sum(pmh_ctx ctx, int nb, const double *row_host, double *out_host)
{
  PMH_ARG(ctx && out_host && nb >= 0 && nb <= 512 && (row_host || !nb));
  double *d = nullptr; // the row, then the 64 lanes' answers
  PMH_CHK(pmh_malloc(ctx, sizeof(double) * (512 + 64), (void **)&d));
  int rc = pmh_memcpy_h2d(ctx, d, row_host, sizeof(double) * (size_t)nb);
  if (!rc) {
    hipLaunchKernelGGL(k_test_block_sum, dim3(1), dim3(64), 0, ctx->stream, (const double *)d, nb, d + 512);
    if (hipGetLastError() != hipSuccess) rc = pmh_set_error(PMH_ERR_HIP, "pmh_mpgp_test_block_sum: the launch failed");
  }
  if (!rc) rc = pmh_memcpy_d2h(ctx, out_host, d + 512, sizeof(double) * 64);
  pmh_free(ctx, d);
  return rc;
}

__global__ __launch_bounds__(PMH_EMIT_TILE) void k_test_block_partials(long long n, const double *__restrict__ a, const double *__restrict__ b, const double *__restrict__ c, double *__restrict__ partials, double *__restrict__ h_partials, int ld)
{
  const long long i    = (long long)blockIdx.x * PMH_EMIT_TILE + threadIdx.x;
  const double    v[3] = {i < n ? a[i] : 0.0, i < n ? b[i] : 0.0, i < n ? c[i] : INFINITY};
  const int       op[3] = {PMH_RED_SUM, PMH_RED_SUM, PMH_RED_MIN};
  pmh_block_partials<3>(v, op, partials, h_partials, ld);
}

extern "C" int pmh_mpgp_test_block_partials(pmh_ctx ctx, int n, const double *a, const double *b, const double *c, double *dev_host, double *pinned_host)
{
  PMH_ARG(ctx && n >= 1 && n <= 512 * PMH_EMIT_TILE && a && b && c && dev_host && pinned_host);
  const int nb = (n + PMH_EMIT_TILE - 1) / PMH_EMIT_TILE, ld = ctx->partials_cap;
  PMH_CHK(pmh_sync(ctx));
  for (int k = 0; k < 3; k++) {
    PMH_CHK(pmh_memcpy_h2d(ctx, ctx->d_partials + (size_t)k * ld, dev_host + (size_t)k * nb, sizeof(double) * (size_t)nb));
    memcpy(ctx->h_partials + (size_t)k * ld, pinned_host + (size_t)k * nb, sizeof(double) * (size_t)nb);
  }
  hipLaunchKernelGGL(k_test_block_partials, dim3(nb), dim3(PMH_EMIT_TILE), 0, ctx->stream, (long long)n, a, b, c, ctx->d_partials, ctx->h_partials, ld);
  PMH_HIP(hipGetLastError());
  PMH_CHK(pmh_sync(ctx));
  for (int k = 0; k < 3; k++) {
    PMH_CHK(pmh_memcpy_d2h(ctx, dev_host + (size_t)k * nb, ctx->d_partials + (size_t)k * ld, sizeof(double) * (size_t)nb));
    memcpy(pinned_host + (size_t)k * nb, ctx->h_partials + (size_t)k * ld, sizeof(double) * (size_t)nb);
  }
  return PMH_SUCCESS;
}

// through the launchers the drivers use: the argument struct, the emission arguments as emit_try asks for them, the phase, the driver's finalising launch
static int test_phase_launch(pmh_ctx ctx, int phase, int n, pmh_mpgp_phase_test *t, int *d_ctl, double *d_ring)
{
  const phase_vecs v = {t->x, t->g, t->p, t->Ap, t->gf, t->lb, t->ub, t->astol};
  const int        nblocks = t->emit ? (n > 0 ? emit_blocks(n) : 0) : vec_blocks(n);
  const int       *halt    = t->use_ctl ? d_ctl + CTL_HALT : nullptr;
  int             *post    = t->use_ctl ? d_ctl + CTL_ITER : nullptr;
  pmh_spec_args    sa      = {};
  if (t->spec) {
    sa.ctl = d_ctl, sa.ring = d_ring, sa.ring_cap = t->ring_cap, sa.max_it = t->max_it;
    sa.ttol = t->ttol, sa.divtol_rhs = t->divtol_rhs, sa.gamma2 = t->gamma2;
  }
  // a chained operator's emission: the kernel of this phase writes x (wx) and / or p (wp); without an operator the tile variant runs with nothing to emit
  pmh_emit_args        eargs = g_noea;
  const pmh_emit_args *ea    = t->emit ? &eargs : nullptr;
  if (t->emit && t->op) {
    const bool wx = phase == PMH_PHASE_EXPANSION || phase == PMH_PHASE_STEP, wp = phase == PMH_PHASE_SPLIT || phase == PMH_PHASE_DIR || phase == PMH_PHASE_PROP_DIR || (phase == PMH_PHASE_STEP && t->setp);
    if (t->op->emit_begin(wx ? t->x : nullptr, wp ? t->p : nullptr, &eargs) != PMH_SUCCESS) return pmh_set_error(PMH_ERR_SUP, "pmh_mpgp_test_phase: the operator does not run on the dual-space chain");
  }
  int group = 0; // the rows the driver's finalising launch of this phase reduces (owed_sums), -1: the objective's one sum
  switch (phase) {
  case PMH_PHASE_SPLIT: PMH_CHK(phase_split(ctx, n, v, ea)); group = owed_sums::SPLIT; break;
  case PMH_PHASE_STEP: PMH_CHK(phase_step(ctx, n, v, t->setp != 0, t->spec ? &sa : nullptr, ea, t->acg_host, t->nb)); group = owed_sums::SPLIT; break;
  case PMH_PHASE_DIR: PMH_CHK(phase_dir(ctx, n, v, halt, ea, t->nb, t->pAp_host)); break;
  case PMH_PHASE_PROP_DIR: PMH_CHK(phase_prop_dir(ctx, n, v, ea)); break;
  case PMH_PHASE_EXPANSION: PMH_CHK(phase_expansion(ctx, n, v, t->afeas, t->alpha, ea)); break;
  case PMH_PHASE_P1_DOTS: PMH_CHK(phase_p1_dots(ctx, n, v)); group = owed_sums::P1; break;
  case PMH_PHASE_THREE_NORMS: PMH_CHK(phase_three_norms(ctx, n, t->x, t->g, t->gf)); group = owed_sums::SPLIT; break;
  case PMH_PHASE_OBJ: PMH_CHK(phase_obj(ctx, n, t->x, t->g, t->b)); group = -1; break;
  }
  if (!t->finalize) return PMH_SUCCESS;
  if (group == owed_sums::SPLIT) return owed_sums::finalize(ctx, owed_sums::SPLIT, 0, nblocks, halt, post);
  if (group == owed_sums::P1) return owed_sums::finalize(ctx, owed_sums::P1, 0, nblocks);
  return finalize_obj(ctx, nblocks);
}

extern "C" int pmh_mpgp_test_phase(pmh_ctx ctx, int phase, int n, pmh_mpgp_phase_test *t)
{
  PMH_ARG(ctx && t && n >= 0 && phase >= PMH_PHASE_SPLIT && phase <= PMH_PHASE_OBJ && t->partials_dev && t->partials_pinned);
  PMH_ARG(!t->emit || (phase <= PMH_PHASE_EXPANSION && n <= 512 * PMH_EMIT_TILE && t->nb >= 0 && t->nb <= 512));
  PMH_ARG(!t->spec || (phase == PMH_PHASE_STEP && t->use_ctl && !t->setp && !t->emit && t->ring_cap >= 0 && t->ring_cap <= 16 && t->ctl[CTL_ITER] >= t->ctl[CTL_BASE]));
  PMH_ARG(!t->op || (t->emit && t->op->n == n));
  PMH_ARG(!t->finalize || phase == PMH_PHASE_SPLIT || phase == PMH_PHASE_STEP || phase >= PMH_PHASE_P1_DOTS);
  // the operands the kernel of this phase dereferences
  const bool nx = phase != PMH_PHASE_DIR, ng = phase != PMH_PHASE_DIR, np = phase <= PMH_PHASE_P1_DOTS, nap = phase == PMH_PHASE_STEP || phase == PMH_PHASE_EXPANSION || phase == PMH_PHASE_P1_DOTS;
  const bool ngf = phase <= PMH_PHASE_DIR || phase == PMH_PHASE_THREE_NORMS;
  PMH_ARG(n == 0 || ((!nx || t->x) && (!ng || t->g) && (!np || t->p) && (!nap || t->Ap) && (!ngf || t->gf) && (phase != PMH_PHASE_OBJ || t->b)));
  const size_t pbytes = sizeof(double) * PMH_MAX_RED * (size_t)ctx->partials_cap;
  PMH_CHK(pmh_sync(ctx));
  int    *d_ctl  = nullptr;
  double *d_ring = nullptr;
  PMH_CHK(pmh_malloc(ctx, sizeof(int) * CTL_NWORDS, (void **)&d_ctl));
  int rc = pmh_malloc(ctx, sizeof(double) * 48, (void **)&d_ring);
  if (!rc) rc = pmh_memcpy_h2d(ctx, d_ctl, t->ctl, sizeof(int) * CTL_NWORDS);
  if (!rc) rc = pmh_memcpy_h2d(ctx, d_ring, t->ring, sizeof(double) * 48);
  if (!rc) rc = pmh_memcpy_h2d(ctx, ctx->d_partials, t->partials_dev, pbytes);
  if (!rc) rc = pmh_memcpy_h2d(ctx, ctx->d_scal, t->scal_dev, sizeof(double) * PMH_NSCAL);
  if (!rc) {
    memcpy(ctx->h_partials, t->partials_pinned, pbytes);
    memcpy(ctx->h_scal, t->scal_pinned, sizeof(double) * PMH_NSCAL);
    rc = test_phase_launch(ctx, phase, n, t, d_ctl, d_ring);
  }
  if (!rc && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = pmh_set_error(PMH_ERR_HIP, "pmh_mpgp_test_phase: stream synchronisation failed");
  if (!rc) rc = pmh_memcpy_d2h(ctx, t->ctl, d_ctl, sizeof(int) * CTL_NWORDS);
  if (!rc) rc = pmh_memcpy_d2h(ctx, t->ring, d_ring, sizeof(double) * 48);
  if (!rc) rc = pmh_memcpy_d2h(ctx, t->partials_dev, ctx->d_partials, pbytes);
  if (!rc) rc = pmh_memcpy_d2h(ctx, t->scal_dev, ctx->d_scal, sizeof(double) * PMH_NSCAL);
  if (!rc) {
    memcpy(t->partials_pinned, ctx->h_partials, pbytes);
    memcpy(t->scal_pinned, ctx->h_scal, sizeof(double) * PMH_NSCAL);
  }
  if (d_ring) pmh_free(ctx, d_ring);
  pmh_free(ctx, d_ctl);
  return rc;
}

// the carried gradient as smalxe.hip hands it over: g (device, n doubles) goes into the solver's work[3] and the next fused solve takes it as A x - b at its starting point
extern "C" int pmh_mpgp_test_set_gradient_valid(pmh_mpgp s, const double *g)
{
  PMH_ARG(s && g && use_fused(s));
  PMH_CHK(ensure_work(s, 3));
  PMH_CHK(pmh_memcpy_d2d(s->ctx, s->work[3], g, sizeof(double) * (size_t)s->n));
  PMH_CHK(pmh_mpgp_set_gradient_valid(s, 1, nullptr));
  return s->g_valid ? PMH_SUCCESS : pmh_set_error(PMH_ERR_STATE, "pmh_mpgp_test_set_gradient_valid: the solver did not take the gradient");
}

// the speculative chain's host-side words after a solve: words[0] = 1 where the solver set the chain up (it does so only where it may use it), words[1..4] = halt,
// iteration, ncg, base as the last batch left them
extern "C" int pmh_mpgp_test_spec_words(pmh_mpgp s, int words[5])
{
  PMH_ARG(s && words);
  PMH_CHK(pmh_sync(s->ctx));
  words[0] = s->d_ctl != nullptr;
  for (int k = 0; k < CTL_NWORDS; k++) words[1 + k] = s->h_ctl ? s->h_ctl[k] : 0;
  return PMH_SUCCESS;
}
