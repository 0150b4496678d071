// PCDUAL dirichlet on gfx950: the Dirichlet preconditioner of the FETI dual operator, y = B S B' x.
//
// The reference's PCApply_Dual (src/pc/impls/dual/pcdual.c:63-78) is y = At' C_bb At x with a matrix C_bb in the middle (logged as
// PC_Dual_MatMultSchur); PCSetUp_Dual (:105-116) fills it for `lumped` only, C_bb = K.  The Dirichlet preconditioner is the same apply
// with C_bb = S = blockdiag(S_b), S_b = K_GG - K_GI K_II^{-1} K_IG the Schur complement of block b on Gamma_b (the dofs B touches,
// exactly as pmh_fexplicit_create takes them) against the rest of the block, I_b.  B S B' only ever sees S_b on Gamma_b, so S lives in
// the dense blocks of a pmh_fexplicit (W_b = S_b, FULL or SYM storage) and one apply is that operator's Bhat' gather, dense GEMV / SYMV
// and Bhat scatter (pmh_fexplicit_mult): 8 (FULL) or 4 (SYM) sum_b n_Gamma_b^2 bytes streamed once.
//
// Set-up, one column gamma of every block per batch (batch k: the k-th dof of every Gamma_b):
//   u = e_gamma;  rhs_I = -(K u)|_I;  K_II u_I = rhs_I (block CG with Jacobi, one block per subdomain that has an interior);
//   u|_I = u_I;  row k of S_b = (K u)|_Gamma_b.
// K u is the CSR product of the block-diagonal K (pmh_blockdiag_mult), the gathers / scatters / row writes are the kernels below, and
// the interior solves share one pmh_matinv over blockdiag(K_II,b), so every batch costs one application of it.  A block without an interior
// gets S_b = K_b[Gamma_b, Gamma_b] and no solve.  The rows are averaged with their transposes when they are stored
// (pmh_fexplicit_store_symmetrized): S is exactly symmetric, as the preconditioned CG needs.
#include <algorithm>
#include <chrono>
#include <vector>

#include "feti_internal.h"
#include "pmh_internal.h"

namespace {
struct PcDualDirichletOp : pmh_op_s {
  pmh_fexplicit E = nullptr;
  long long     n_solves = 0;
  double        setup_seconds = 0.0;
  ~PcDualDirichletOp() override { pmh_fexplicit_destroy(E); }
  int mult(const double *x, double *y) override { return pmh_fexplicit_mult(E, x, y); } // PCApply_Dual pcdual.c:63-78 with C_bb = S
  int mult_transpose(const double *x, double *y) override { return mult(x, y); }     // B S B' is symmetric
};

// what the set-up allocates; released on every exit
struct PdWork {
  pmh_ctx       ctx = nullptr;
  pmh_csr       Kii = nullptr;
  pmh_blockdiag KIIb = nullptr;
  pmh_matinv    M = nullptr;
  double       *u = nullptr, *y = nullptr, *rhs = nullptr, *sol = nullptr, *S = nullptr;
  int          *d_goff = nullptr, *d_grel = nullptr, *d_iglob = nullptr;
  long long    *d_soff = nullptr;
  ~PdWork()
  {
    pmh_matinv_destroy(M);
    pmh_blockdiag_destroy(KIIb);
    pmh_csr_destroy(Kii);
    for (void *p : {(void *)u, (void *)y, (void *)rhs, (void *)sol, (void *)S, (void *)d_goff, (void *)d_grel, (void *)d_iglob, (void *)d_soff})
      if (p) pmh_free(ctx, p);
  }
};
} // namespace

// u[rowstart_b + gamma_b[k]] = 1 for every block with more than k dofs in Gamma_b (one thread per block)
__global__ void k_pd_unit(int nb, int k, const int *__restrict__ goff, const int *__restrict__ grel, const int *__restrict__ rs, double *__restrict__ u)
{
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < nb && k < goff[b + 1] - goff[b]) u[rs[b] + grel[goff[b] + k]] = 1.0;
}

// rhs_I = -(K u)|_I in the numbering of blockdiag(K_II,b)
__global__ __launch_bounds__(PMH_BLOCK) void k_pd_gather_neg(int nI, const int *__restrict__ iglob, const double *__restrict__ y, double *__restrict__ rhs)
{
  for (int i = blockIdx.x * PMH_BLOCK + threadIdx.x; i < nI; i += gridDim.x * PMH_BLOCK) rhs[i] = -y[iglob[i]];
}

// u|_I = u_I
__global__ __launch_bounds__(PMH_BLOCK) void k_pd_scatter(int nI, const int *__restrict__ iglob, const double *__restrict__ sol, double *__restrict__ u)
{
  for (int i = blockIdx.x * PMH_BLOCK + threadIdx.x; i < nI; i += gridDim.x * PMH_BLOCK) u[iglob[i]] = sol[i];
}

// row k of S_b (n_b x n_b row-major at S + soff[b]) = (K u)|_Gamma_b; blockIdx.y = block
__global__ __launch_bounds__(PMH_BLOCK) void k_pd_row(int k, const int *__restrict__ goff, const int *__restrict__ grel, const int *__restrict__ rs, const long long *__restrict__ soff,
                                                      const double *__restrict__ y, double *__restrict__ S)
{
  const int b = blockIdx.y, n = goff[b + 1] - goff[b];
  if (k >= n) return;
  double *row = S + soff[b] + (long long)k * n;
  for (int q = blockIdx.x * PMH_BLOCK + threadIdx.x; q < n; q += gridDim.x * PMH_BLOCK) row[q] = y[rs[b] + grel[goff[b] + q]];
}

static int pd_assemble(PcDualDirichletOp *o, pmh_gluing B, pmh_blockdiag K, double rtol, int max_it)
{
  pmh_ctx   ctx = B->ctx;
  const int nb = K->nblocks, n = K->n;
  PdWork    w;
  w.ctx = ctx;
  // Gamma_b as the explicit operator found it (block-relative, ascending)
  std::vector<int> ngam(nb), goff(nb + 1, 0), grel;
  PMH_CHK(pmh_fexplicit_sizes(o->E, nullptr, ngam.data(), nullptr, nullptr));
  for (int b = 0; b < nb; b++) {
    std::vector<int> g((size_t)std::max(1, ngam[b]));
    PMH_CHK(pmh_fexplicit_get_block(o->E, b, nullptr, g.data()));
    for (int i = 0; i < ngam[b]; i++) grel.push_back(g[i] - K->rowstart[b]);
    goff[b + 1] = (int)grel.size();
  }
  // blockdiag(K_II,b) on the host from the device copy of K: the blocks that have an interior, in block order
  std::vector<int>    rp((size_t)n + 1), ci((size_t)std::max(1LL, K->K->nnz));
  std::vector<double> va((size_t)std::max(1LL, K->K->nnz));
  PMH_CHK(pmh_memcpy_d2h(ctx, rp.data(), K->K->d_rowptr, sizeof(int) * rp.size()));
  if (K->K->nnz) {
    PMH_CHK(pmh_memcpy_d2h(ctx, ci.data(), K->K->d_col, sizeof(int) * (size_t)K->K->nnz));
    PMH_CHK(pmh_memcpy_d2h(ctx, va.data(), K->K->d_val, sizeof(double) * (size_t)K->K->nnz));
  }
  std::vector<int> imap((size_t)std::max(1, n), -1), iglob, irs(1, 0);
  std::vector<char> interior(nb, 0);
  for (int b = 0; b < nb; b++) {
    std::vector<char> inG((size_t)std::max(1, K->rowstart[b + 1] - K->rowstart[b]), 0);
    for (int k = goff[b]; k < goff[b + 1]; k++) inG[grel[k]] = 1;
    for (int i = K->rowstart[b]; i < K->rowstart[b + 1]; i++)
      if (!inG[i - K->rowstart[b]]) imap[i] = (int)iglob.size(), iglob.push_back(i);
    if ((int)iglob.size() > irs.back()) irs.push_back((int)iglob.size()), interior[b] = 1;
  }
  const int nI = (int)iglob.size();
  if (nI) {
    std::vector<int>    irp(1, 0), ici;
    std::vector<double> iva;
    for (int i : iglob) {
      for (int k = rp[i]; k < rp[i + 1]; k++)
        if (imap[ci[k]] >= 0) ici.push_back(imap[ci[k]]), iva.push_back(va[k]);
      irp.push_back((int)ici.size());
    }
    PMH_CHK(pmh_csr_create(ctx, nI, nI, irp.data(), ici.data(), iva.data(), &w.Kii));
    PMH_CHK(pmh_blockdiag_create(ctx, (int)irs.size() - 1, irs.data(), w.Kii, &w.KIIb));
    PMH_CHK(pmh_matinv_create(w.KIIb, rtol, 1e-300, max_it, 1, &w.M)); // Jacobi PCG per block; a block idle in a batch has rhs 0 and stays out of the iteration
  }
  // device work: u, K u, the interior vectors, the rows of every S_b
  std::vector<long long> soff(nb);
  long long              stot = 0;
  for (int b = 0; b < nb; b++) soff[b] = stot, stot += (long long)ngam[b] * ngam[b];
  const size_t bx = sizeof(double) * (size_t)std::max(1, n), bi = sizeof(double) * (size_t)std::max(1, nI);
  PMH_CHK(pmh_malloc(ctx, bx, (void **)&w.u));
  PMH_CHK(pmh_malloc(ctx, bx, (void **)&w.y));
  PMH_CHK(pmh_malloc(ctx, bi, (void **)&w.rhs));
  PMH_CHK(pmh_malloc(ctx, bi, (void **)&w.sol));
  PMH_CHK(pmh_malloc(ctx, sizeof(double) * (size_t)std::max(1LL, stot), (void **)&w.S));
  PMH_CHK(pmh_malloc(ctx, sizeof(int) * (size_t)(nb + 1), (void **)&w.d_goff));
  PMH_CHK(pmh_malloc(ctx, sizeof(int) * (size_t)std::max<size_t>(1, grel.size()), (void **)&w.d_grel));
  PMH_CHK(pmh_malloc(ctx, sizeof(int) * (size_t)std::max(1, nI), (void **)&w.d_iglob));
  PMH_CHK(pmh_malloc(ctx, sizeof(long long) * (size_t)std::max(1, nb), (void **)&w.d_soff));
  PMH_CHK(pmh_memcpy_h2d(ctx, w.d_goff, goff.data(), sizeof(int) * (size_t)(nb + 1)));
  if (!grel.empty()) PMH_CHK(pmh_memcpy_h2d(ctx, w.d_grel, grel.data(), sizeof(int) * grel.size()));
  if (nI) PMH_CHK(pmh_memcpy_h2d(ctx, w.d_iglob, iglob.data(), sizeof(int) * (size_t)nI));
  if (nb) PMH_CHK(pmh_memcpy_h2d(ctx, w.d_soff, soff.data(), sizeof(long long) * (size_t)nb));
  const int   nbatch = nb ? *std::max_element(ngam.begin(), ngam.end()) : 0;
  hipStream_t st     = ctx->stream;
  const dim3  gI((unsigned)std::max(1, std::min(1024, (nI + PMH_BLOCK - 1) / PMH_BLOCK)));
  long long   n_solves = 0;
  for (int k = 0; k < nbatch; k++) {
    PMH_HIP(hipMemsetAsync(w.u, 0, bx, st));
    hipLaunchKernelGGL(k_pd_unit, dim3((nb + 63) / 64), dim3(64), 0, st, nb, k, (const int *)w.d_goff, (const int *)w.d_grel, (const int *)K->d_rowstart, w.u);
    PMH_HIP(hipGetLastError());
    bool solved = false;
    for (int b = 0; b < nb && !solved; b++) solved = interior[b] && k < ngam[b];
    if (solved) { // u_I = -K_II^{-1} (K e_gamma)|_I
      PMH_CHK(pmh_blockdiag_mult(K, w.u, w.y));
      hipLaunchKernelGGL(k_pd_gather_neg, gI, dim3(PMH_BLOCK), 0, st, nI, (const int *)w.d_iglob, (const double *)w.y, w.rhs);
      PMH_HIP(hipGetLastError());
      PMH_CHK(pmh_matinv_mult(w.M, w.rhs, w.sol));
      if (w.M->last_max_its >= w.M->max_it)
        return pmh_set_error(PMH_ERR_STATE, "pmh_op_create_pc_dual_dirichlet: an interior solve of batch %d did not reach rtol %.1e within %d iterations", k, rtol, w.M->max_it);
      hipLaunchKernelGGL(k_pd_scatter, gI, dim3(PMH_BLOCK), 0, st, nI, (const int *)w.d_iglob, (const double *)w.sol, w.u);
      PMH_HIP(hipGetLastError());
      for (int b = 0; b < nb; b++) n_solves += (interior[b] && k < ngam[b]) ? 1 : 0;
    }
    PMH_CHK(pmh_blockdiag_mult(K, w.u, w.y));
    hipLaunchKernelGGL(k_pd_row, dim3((unsigned)std::max(1, std::min(64, (nbatch + PMH_BLOCK - 1) / PMH_BLOCK)), (unsigned)nb), dim3(PMH_BLOCK), 0, st, k, (const int *)w.d_goff,
                       (const int *)w.d_grel, (const int *)K->d_rowstart, (const long long *)w.d_soff, (const double *)w.y, w.S);
    PMH_HIP(hipGetLastError());
  }
  for (int b = 0; b < nb; b++) PMH_CHK(pmh_fexplicit_store_symmetrized(o->E, b, w.S + soff[b], std::max(1, ngam[b])));
  PMH_CHK(pmh_sync(ctx));
  o->n_solves = n_solves;
  return PMH_SUCCESS;
}

extern "C" int pmh_op_create_pc_dual_dirichlet(pmh_gluing B, pmh_blockdiag K, int storage, double rtol, int max_it, pmh_op *op)
{
  PMH_ARG(B && K && op && B->n_x == K->n && rtol > 0.0 && max_it > 0);
  if (storage == PMH_FX_CLASS || storage == PMH_FX_CLASS_SYM || storage == PMH_FX_CLASS_ORBIT)
    return pmh_set_error(PMH_ERR_SUP, "pmh_op_create_pc_dual_dirichlet: class-shared storage is not built (PMH_FX_FULL / PMH_FX_SYM)");
  PMH_ARG(storage == PMH_FX_FULL || storage == PMH_FX_SYM);
  if (pmh_comm_on(B->ctx)) return pmh_set_error(PMH_ERR_SUP, "pmh_op_create_pc_dual_dirichlet: several GPUs are not built");
  auto               t0 = std::chrono::steady_clock::now();
  PcDualDirichletOp *o  = new PcDualDirichletOp();
  o->ctx = B->ctx, o->n = B->n_lambda;
  int rc = pmh_fexplicit_create(B, K, storage, &o->E);
  if (!rc) rc = pd_assemble(o, B, K, rtol, max_it);
  if (!rc) {
    o->setup_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    rc = pmh_fexplicit_mark_assembled(o->E, o->n_solves, o->setup_seconds);
  }
  if (rc) {
    delete o;
    return rc;
  }
  *op = o;
  return PMH_SUCCESS;
}

static int pd_cast(pmh_op op, PcDualDirichletOp **o)
{
  PMH_ARG(op);
  *o = dynamic_cast<PcDualDirichletOp *>(op);
  if (!*o) return pmh_set_error(PMH_ERR_ARG, "not an operator of pmh_op_create_pc_dual_dirichlet");
  return PMH_SUCCESS;
}

extern "C" int pmh_pc_dual_dirichlet_stats(pmh_op op, long long *n_solves, double *setup_seconds, double *dense_bytes)
{
  PcDualDirichletOp *o;
  PMH_CHK(pd_cast(op, &o));
  if (n_solves) *n_solves = o->n_solves;
  if (setup_seconds) *setup_seconds = o->setup_seconds;
  if (dense_bytes) {
    long long db = 0;
    PMH_CHK(pmh_fexplicit_sizes(o->E, nullptr, nullptr, &db, nullptr));
    *dense_bytes = (double)db;
  }
  return PMH_SUCCESS;
}

extern "C" int pmh_pc_dual_dirichlet_get_block(pmh_op op, int b, double *S_host, int *gamma_host)
{
  PcDualDirichletOp *o;
  PMH_CHK(pd_cast(op, &o));
  return pmh_fexplicit_get_block(o->E, b, S_host, gamma_host);
}

extern "C" int pmh_pc_dual_dirichlet_get_explicit(pmh_op op, pmh_fexplicit *E)
{
  PcDualDirichletOp *o;
  PMH_CHK(pd_cast(op, &o));
  PMH_ARG(E);
  *E = o->E;
  return PMH_SUCCESS;
}
