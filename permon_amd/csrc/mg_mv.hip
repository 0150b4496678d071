// Multi-right-hand-side K^+, part 2: the V-cycle of mg.hip on interleaved multivectors of R = PMH_MV_R columns (see mv_internal.h).
//
// The hierarchy is the one pmh_mg holds (level operators as CSR, node-wise transfer operators, Jacobi scaling, Chebyshev constants, dense coarse
// pseudo-inverses): nothing is set up twice but the ELL copies of the level operators (built on the device, mv.hip) and the work multivectors.  The cycle is
// the fused form of mg.hip (mg_fused_level, mg_internal.h: one driver for both): degree-2 Chebyshev/Jacobi smoothing finished inside the operator kernel, fp32 vectors, level operators in the
// precision pmh_mg keeps them in (fp16 on the finest levels by default).  Per smoothed level: d0 | PRE | SUB | restrict (+ the coarse d0) | ... |
// prolong-subtract | POST1 | POST2.  The transfers are node-wise where P = P_node (x) I_3 (the box hierarchies) and scalar CSR otherwise (smoothed aggregation).  A
// hierarchy of another shape (fp64 cycle, other degree, a level without 3 x 3 blocks) is refused (PMH_EPI_UNSUPPORTED, no error recorded): the caller keeps the
// one-column solver.
#include "mg_transfer.h"
#include "mv_internal.h"

#define MV_R PMH_MV_R
typedef float mvg_flt4 __attribute__((ext_vector_type(4)));
static_assert(MV_R == 8, "k_mg_restrict<float, 8, 1, 8, 1>: 8 entry groups x 8 columns per wavefront");

struct mg_mv_level {
  pmh_mv_ell E = nullptr;
  pmh_mv_ell EP = nullptr, ER = nullptr; // a prolongation that is not node-wise as 3 x 3 blocks: -P and P' (fp32 entries), else NULL (node-wise / scalar kernels)
  float     *x = nullptr, *b = nullptr, *r = nullptr, *d = nullptr, *t = nullptr, *xa = nullptr;
};
struct pmh_mg_mv_s {
  pmh_mg                   mg;
  pmh_ctx                  ctx; // (kept: the caller may destroy the pmh_mg before this object)
  // > 1: every level is block diagonal with nrep congruent blocks and this object works on the FIRST one (a prefix of every array of pmh_mg)
  int                      nrep = 1;
  std::vector<mg_mv_level> L;
};

// max |pinv_b - pinv_0| over the coarse blocks b > 0 (fp16 or fp32 entries, equal sizes): the coarse inverses of congruent blocks must be equal too
template <typename TP> __global__ __launch_bounds__(PMH_BLOCK) void k_mvg_pinv_diff(int nb, long long m2, const TP *__restrict__ pinv,
                        int *__restrict__ differs)
{
  for (long long i = (long long)blockIdx.x * PMH_BLOCK + threadIdx.x; i < m2; i += (long long)gridDim.x * PMH_BLOCK)
    for (int b = 1; b < nb; b++)
      if ((float)pinv[(long long)b * m2 + i] != (float)pinv[i]) *differs = 1;
}

// d0 = D^-1 b / theta (and the fp32 copy of an fp64 b): one thread per 4 consecutive entries of a row's R columns
template <typename TB>
__global__ __launch_bounds__(PMH_BLOCK) void k_mvg_d0(long long nR, const int *__restrict__ halt, const float *__restrict__ dinv, const TB *__restrict__ b,
                        float itheta, float *__restrict__ d, float *__restrict__ bcopy)
{
  if (halt && *halt) return;
  for (long long i = 4 * ((long long)blockIdx.x * PMH_BLOCK + threadIdx.x); i < nR; i += 4LL * gridDim.x * PMH_BLOCK) {
    const float di = dinv[i / MV_R] * itheta;
    float       v[4];
#pragma unroll
    for (int k = 0; k < 4; k++) v[k] = (float)b[i + k];
    if (bcopy) *(mvg_flt4 *)(bcopy + i) = mvg_flt4{v[0], v[1], v[2], v[3]};
    *(mvg_flt4 *)(d + i) = mvg_flt4{di * v[0], di * v[1], di * v[2], di * v[3]};
  }
}

// coarsest level: X_b = pinv_b B_b for the R columns: one wavefront per row of the dense block, lanes stride the row, R sums per lane
template <typename TP>
__global__ __launch_bounds__(PMH_BLOCK) void k_mvg_coarse(int nb, int n, const int *__restrict__ halt, const int *__restrict__ rs,
                        const long long *__restrict__ ofs, const TP *__restrict__ pinv, float scale, const float *__restrict__ b,
                                                         float *__restrict__ x)
{
  if (halt && *halt) return;
  const int lane = threadIdx.x & 63;
  const int row  = blockIdx.x * (PMH_BLOCK / 64) + (threadIdx.x >> 6);
  if (row >= n) return;
  const int    lo = mg_coarse_block(rs, nb, row);
  const int    r0 = rs[lo], m = rs[lo + 1] - r0;
  const TP    *a  = pinv + ofs[lo] + (size_t)(row - r0) * m;
  const float *bb = b + (size_t)r0 * MV_R;
  float        s[MV_R];
#pragma unroll
  for (int r = 0; r < MV_R; r++) s[r] = 0.f;
  for (int j = lane; j < m; j += 64) {
    const float    w  = (float)a[j];
    const mvg_flt4 v0 = *(const mvg_flt4 *)(bb + (size_t)j * MV_R), v1 = *(const mvg_flt4 *)(bb + (size_t)j * MV_R + 4);
    s[0] += w * v0.x, s[1] += w * v0.y, s[2] += w * v0.z, s[3] += w * v0.w;
    s[4] += w * v1.x, s[5] += w * v1.y, s[6] += w * v1.z, s[7] += w * v1.w;
  }
#pragma unroll
  for (int r = 0; r < MV_R; r++)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s[r] += __shfl_down(s[r], o, 64);
  if (lane == 0) {
    float *xo = x + (size_t)row * MV_R;
#pragma unroll
    for (int r = 0; r < MV_R; r++) xo[r] = (sizeof(TP) == 2) ? s[r] * scale : s[r];
  }
}

// The same on the matrix cores (round 6), for the LARGE dense coarse blocks of the one-block regime (5 184 rows on the 43^3 cube: 54 MB of fp16 entries per solve).  The form
// above reads the 32 bytes of B's row j once per ROW of pinv -- 860 MB through the L1s per solve, 35.6 us (1.5 TB/s on the matrix) -- and sums over k with 48 butterfly steps
// per row.  Here a workgroup of MVG_CW wavefronts owns 16 rows, wavefront w the steps [w per, (w+1) per) of 32 k's: lane (i, q) = (l & 15, l >> 4) loads the 8 entries
// pinv[row0 + i][k0 + 8 q ... + 8) in one 16-byte load and feeds them to 8 v_mfma_f32_16x16x4_f32 (exact fp32 FMAs; A[i][k = q] / B[k = q][j = l & 15], k taken as 8 q + e for
// the e-th one: any assignment of k's to the 4 k-slots is a permutation of the sum) against B[k0 + 8 q + e][j & 7] -- the 8 columns twice: half of the instruction's N = 16 is
// idle.  The sum over k happens inside the instruction; the wavefronts' 16 x 8 partials are added through LDS in wave order (fixed).  21.4 us = 2.5 TB/s on the matrix: 324
// workgroups on 256 CUs leave 68 CUs with two.  (The 4x4x1 16-block form -- no idle half, 8- or 4-row workgroups -- was built too: 18.7 - 20.1 us, removed again;
// docs/LAB_NOTEBOOK.md "Round 6" 5, lane maps in scripts/micro/mfma_f32_4x4.hip.)
// Needs every block's size to be a multiple of 16 (rows of a workgroup in ONE block, 16-byte aligned rows); else the form above.
typedef float    mvg_f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 mvg_h8 __attribute__((ext_vector_type(8)));
template <int MVG_CU> struct mvg_cstage {
  mvg_h8   a[MVG_CU];
  mvg_flt4 b[MVG_CU];
};
template <int MVG_CW, int MVG_CU> __global__ __launch_bounds__(64 * MVG_CW) void k_mvg_coarse_mfma(int nb, const int *__restrict__ halt, const int *__restrict__ rs, const long long *__restrict__ ofs,
                        const _Float16 *__restrict__ pinv, float scale, const float *__restrict__ b, float *__restrict__ x)
{
  if (halt && *halt) return;
  __shared__ float part[MVG_CW][16][MV_R];
  __shared__ float tr[MVG_CW][MVG_CU][4 * 8 * 8]; // per wavefront and step: the 32 x 8 entries of B, [q][column][k & 7]
  const int        row0 = blockIdx.x * 16;
  const int        lo = mg_coarse_block(rs, nb, row0);
  const int       r0 = rs[lo], m = rs[lo + 1] - r0;
  const int       lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, q = lane >> 4, jr = i & 7, h = i >> 3;
  const _Float16 *a  = pinv + ofs[lo] + (size_t)(row0 - r0 + i) * m + 8 * q;
  // B[k0 + 8 q ... + 8)[0 ... 8) is 256 contiguous bytes: lane (jr, h) of the 16 with this q brings 16 of them (row jr, columns 4 h ... 4 h + 3) -- ONE coalesced load per
  // step where every lane fetching its own 8 operands (column jr of the 8 rows) took 8 and left the kernel bound by the address rate of those (26 us)
  const float *bb = b + ((size_t)r0 + 8 * q + jr) * MV_R + 4 * h;
  const int    nsteps = (m + 31) / 32, per = (nsteps + MVG_CW - 1) / MVG_CW;
  const int    s0 = wave * per, s1 = min(nsteps, s0 + per);
  auto         load = [&](mvg_cstage<MVG_CU> &S, int s) {
#pragma unroll
    for (int u = 0; u < MVG_CU; u++) {
      const int  k0 = 32 * (s + u);
      const bool ok = (s + u < s1) && (k0 + 8 * q < m); // (m % 8 == 0: the 8 entries are in the row or not)
      if (ok) {
        S.a[u] = *(const mvg_h8 *)(a + k0);
        S.b[u] = *(const mvg_flt4 *)(bb + (size_t)k0 * MV_R);
      } else {
        S.a[u] = mvg_h8{0, 0, 0, 0, 0, 0, 0, 0};
        S.b[u] = mvg_flt4{0.f, 0.f, 0.f, 0.f};
      }
    }
  };
  mvg_f32x4 c0 = {0.f, 0.f, 0.f, 0.f}, c1 = {0.f, 0.f, 0.f, 0.f}; // two chains: the instruction's dependent latency (40 cycles) is above its issue time (32)
  auto      mults = [&](const mvg_cstage<MVG_CU> &S) {
    // the 8 x 8 blocks transposed through the wavefront's own LDS lines (its LDS operations execute in order: no barrier, the compiler is only kept from reordering them)
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int u = 0; u < MVG_CU; u++) {
      float *t = &tr[wave][u][(q * 8 + 4 * h) * 8 + jr];
      t[0] = S.b[u].x, t[8] = S.b[u].y, t[16] = S.b[u].z, t[24] = S.b[u].w;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int u = 0; u < MVG_CU; u++) {
      const mvg_flt4 v0 = *(const mvg_flt4 *)&tr[wave][u][(q * 8 + jr) * 8], v1 = *(const mvg_flt4 *)&tr[wave][u][(q * 8 + jr) * 8 + 4];
      c0 = __builtin_amdgcn_mfma_f32_16x16x4f32((float)S.a[u][0], v0.x, c0, 0, 0, 0);
      c1 = __builtin_amdgcn_mfma_f32_16x16x4f32((float)S.a[u][1], v0.y, c1, 0, 0, 0);
      c0 = __builtin_amdgcn_mfma_f32_16x16x4f32((float)S.a[u][2], v0.z, c0, 0, 0, 0);
      c1 = __builtin_amdgcn_mfma_f32_16x16x4f32((float)S.a[u][3], v0.w, c1, 0, 0, 0);
      c0 = __builtin_amdgcn_mfma_f32_16x16x4f32((float)S.a[u][4], v1.x, c0, 0, 0, 0);
      c1 = __builtin_amdgcn_mfma_f32_16x16x4f32((float)S.a[u][5], v1.y, c1, 0, 0, 0);
      c0 = __builtin_amdgcn_mfma_f32_16x16x4f32((float)S.a[u][6], v1.z, c0, 0, 0, 0);
      c1 = __builtin_amdgcn_mfma_f32_16x16x4f32((float)S.a[u][7], v1.w, c1, 0, 0, 0);
    }
  };
  mvg_cstage<MVG_CU> S0, S1;
  load(S0, s0);
  for (int s = s0; s < s1; s += 2 * MVG_CU) { // (the loads of the next stage are in flight while this one's products issue)
    load(S1, s + MVG_CU);
    mults(S0);
    load(S0, s + 2 * MVG_CU);
    mults(S1);
  }
  // C[row = 4 q + v][col = i]: columns 8 ... 15 repeat 0 ... 7
  if (i < MV_R) {
#pragma unroll
    for (int v = 0; v < 4; v++) part[wave][4 * q + v][i] = c0[v] + c1[v];
  }
  __syncthreads();
  if (threadIdx.x < 16 * MV_R) {
    const int rr = threadIdx.x / MV_R, cc = threadIdx.x % MV_R;
    float     sum = part[0][rr][cc];
#pragma unroll
    for (int w = 1; w < MVG_CW; w++) sum += part[w][rr][cc];
    x[(size_t)(row0 + rr) * MV_R + cc] = sum * scale;
  }
}

int pmh_mg_mv_destroy(pmh_mg_mv M)
{
  if (!M) return PMH_SUCCESS;
  pmh_ctx ctx = M->ctx;
  for (auto &l : M->L) {
    pmh_mv_ell_destroy(l.E), pmh_mv_ell_destroy(l.EP), pmh_mv_ell_destroy(l.ER);
    pmh_free(ctx, l.x), pmh_free(ctx, l.b), pmh_free(ctx, l.r), pmh_free(ctx, l.d), pmh_free(ctx, l.t), pmh_free(ctx, l.xa);
  }
  delete M;
  return PMH_SUCCESS;
}

int pmh_mg_mv_create(pmh_mg mg, pmh_mg_mv *out, int nrep)
{
  PMH_ARG(mg && out && nrep >= 1);
  *out = nullptr;
  if (nrep > 1) { // congruence of every level as pmh_bsr3_from_csr verified it, equal coarse inverses
    for (int l = 0; l + 1 < mg->nlevels; l++)
      if (!mg->L[l].Ab || mg->L[l].Ab->nrep != nrep) {
        pmh_mv_set_why("the blocks are not congruent on every level of the hierarchy");
        return PMH_EPI_UNSUPPORTED;
      }
    const int nc = mg->L[mg->nlevels - 1].n;
    if (mg->nb_coarse != nrep || nc % nrep) {
      pmh_mv_set_why("the coarse level does not have one block per congruent block");
      return PMH_EPI_UNSUPPORTED;
    }
    int *d_diff, h_diff = 0;
    PMH_CHK(pmh_malloc(mg->ctx, sizeof(int), (void **)&d_diff));
    PMH_HIP(hipMemsetAsync(d_diff, 0, sizeof(int), mg->ctx->stream));
    const long long m2 = (long long)(nc / nrep) * (nc / nrep);
    if (mg->cp_half) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_mvg_pinv_diff<_Float16>), dim3(256), dim3(PMH_BLOCK), 0, mg->ctx->stream, nrep, m2,
                            (const _Float16 *)mg->d_cpinv, d_diff);
    else if (mg->is_float) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_mvg_pinv_diff<float>), dim3(256), dim3(PMH_BLOCK), 0, mg->ctx->stream, nrep, m2,
                            (const float *)mg->d_cpinv, d_diff);
    PMH_CHK(pmh_memcpy_d2h(mg->ctx, &h_diff, d_diff, sizeof(int)));
    pmh_free(mg->ctx, d_diff);
    if (h_diff) {
      pmh_mv_set_why("the coarse pseudo-inverses of the congruent blocks differ");
      return PMH_EPI_UNSUPPORTED;
    }
  }
  if (!(mg->is_float && mg->fused && mg->nlevels > 1 && mg->degree == 2)) {
    pmh_mv_set_why(!mg->is_float ? "the V-cycle runs in fp64" : (mg->degree != 2 ? "the smoother is not of degree 2" : (mg->nlevels < 2 ? "the hierarchy has one level" : "the V-cycle is not the fused form (PMH_MG_FUSED=0 or a level without 3 x 3 blocks)")));
    return PMH_EPI_UNSUPPORTED;
  }
  for (int l = 0; l + 1 < mg->nlevels; l++) {
    const bool nodal = mg->L[l].pn_rowptr && mg->L[l].rn_rowptr;
    if (!mg->L[l].Ab || mg->L[l].n % 3 || (!nodal && (nrep > 1 || !mg->L[l].pv_owned))) { // (a scalar P of congruent blocks: its prefix is not addressed separately here)
      pmh_mv_set_why(!mg->L[l].Ab ? "a level operator has no 3 x 3 block copy" : "a prolongation that is not node-wise (P = P_node (x) I_3) on congruent blocks");
      return PMH_EPI_UNSUPPORTED;
    }
  }
  pmh_ctx   ctx = mg->ctx;
  pmh_mg_mv M   = new pmh_mg_mv_s();
  M->mg = mg, M->ctx = ctx, M->nrep = nrep;
  M->L.resize(mg->nlevels);
  int rc = PMH_SUCCESS;
  for (int l = 0; l < mg->nlevels && !rc; l++) {
    mg_level    &Lv = mg->L[l];
    mg_mv_level &Ml = M->L[l];
    const size_t nR = (size_t)(Lv.n / nrep) * MV_R;
    if (l + 1 < mg->nlevels) {
      rc = pmh_mv_ell_create_prefix(Lv.A, nrep, Lv.Ab->storage == PMH_BSR_F64 ? PMH_BSR_F32 : Lv.Ab->storage, &Ml.E);
      if (!rc && !Ml.E) {
        pmh_mg_mv_destroy(M);
        pmh_mv_set_why("a level operator has rows with unsorted columns or more than 2048 blocks of 3 x 3 in a block row");
        return PMH_EPI_UNSUPPORTED;
      }
      if (!rc && !(Lv.pn_rowptr && Lv.rn_rowptr) && Lv.P->ncols % 3 == 0) { // aggregation hierarchy: P couples a fine node to the 6 dofs of a few aggregates -- two 3 x 3 blocks each
        rc = pmh_mv_ell_create_rect(Lv.P, PMH_BSR_F32, 1, &Ml.EP);
        if (!rc && Ml.EP) rc = pmh_mv_ell_create_rect(Lv.P->transpose, PMH_BSR_F32, 0, &Ml.ER);
        if (!rc && !Ml.ER) pmh_mv_ell_destroy(Ml.EP), Ml.EP = nullptr; // (both or none: the scalar kernels otherwise)
      }
      for (float **v : {&Ml.r, &Ml.d, &Ml.t, &Ml.xa})
        if (!rc) rc = pmh_malloc(ctx, sizeof(float) * nR, (void **)v);
    }
    for (float **v : {&Ml.x, &Ml.b})
      if (!rc) rc = pmh_malloc(ctx, sizeof(float) * nR, (void **)v);
  }
  if (rc) {
    pmh_mg_mv_destroy(M);
    return rc;
  }
  *out = M;
  return PMH_SUCCESS;
}

// which transfer kernels level l launches and which coarse solve the last level (pmh_mg_mv_test_info reports the same numbers): the rectangular ELL pair exists both or none
enum { MVG_COARSE_F32 = 0, MVG_COARSE_F16 = 1, MVG_COARSE_MFMA = 2 };
static inline int mvg_transfer_kind(pmh_mg_mv M, int l)
{
  if (l >= M->mg->nlevels - 1) return MG_TRANSFER_NONE;
  if (M->L[l].ER && M->L[l].EP) return MG_TRANSFER_ELL;
  return M->mg->L[l].rn_rowptr != nullptr ? MG_TRANSFER_NODAL : MG_TRANSFER_SCALAR;
}
static inline int mvg_coarse_kind(pmh_mg mg) { return (mg->cp_half && mg->coarse_m16) ? MVG_COARSE_MFMA : (mg->cp_half ? MVG_COARSE_F16 : MVG_COARSE_F32); }

static int mvg_cycle(pmh_mg_mv M, int l, const double *b64, double *z64, bool d0_ready, const int *halt);

// the 8-column form of mg_fused_level (mg_internal.h): level operators as ELL copies (mv.hip), fp32 multivectors of the first of nrep congruent blocks
struct mg_form8 {
  typedef float T;
  pmh_mg        mg;
  pmh_mg_mv     M;
  const int    *halt;
  mg_vecs<float> vecs(int l) const
  {
    const mg_mv_level &Ml = M->L[l];
    return {Ml.x, Ml.b, Ml.r, Ml.d, Ml.t, Ml.xa};
  }
  void d0(int l, const float *b, const double *b64, const float *dinv, float itheta, float *d) const
  {
    const long long nR = (long long)(mg->L[l].n / M->nrep) * MV_R;
    if (b64) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_mvg_d0<double>), mg_grid(nR / 4), dim3(PMH_BLOCK), 0, mg->ctx->stream, nR, halt, dinv, b64, itheta, d, (float *)b);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_mvg_d0<float>), mg_grid(nR / 4), dim3(PMH_BLOCK), 0, mg->ctx->stream, nR, halt, dinv, b, itheta, d, (float *)nullptr);
  }
  int op(int l, const float *x, float *y, int epi, const pmh_mv_epi<float> &e) const { return pmh_mv_spmv_f32(M->L[l].E, x, y, epi, &e, halt); }
  int restrict_to(int l, const float *t, float *bc, float *dc) const
  {
    const int tk = mvg_transfer_kind(M, l);
    if (tk != MG_TRANSFER_ELL) return mg_restrict<float, MV_R>(mg, l, tk, M->nrep, halt, t, bc, dc);
    pmh_mv_epi<float> er;
    memset(&er, 0, sizeof(er));
    if (dc) er.dinv = (const float *)mg->L[l + 1].dinv, er.d = dc, er.c0 = (float)(1.0 / mg->L[l + 1].theta);
    return pmh_mv_spmv_f32(M->L[l].ER, t, bc, PMH_MV_EPI_RESTRICT, &er, halt);
  }
  int prolong_sub(int l, const float *xc, float *x) const
  {
    const int tk = mvg_transfer_kind(M, l);
    if (tk != MG_TRANSFER_ELL) return mg_prolong_sub<float, MV_R>(mg, l, tk, M->nrep, halt, xc, x);
    pmh_mv_epi<float> ep;
    memset(&ep, 0, sizeof(ep));
    ep.y1 = x;
    return pmh_mv_spmv_f32(M->L[l].EP, xc, x, PMH_EPI_ADD, &ep, halt); // x += (-P) x_c
  }
  int descend(int l, const float *, float *, bool d0_ready) const { return mvg_cycle(M, l, nullptr, nullptr, d0_ready, halt); } // (b and x are the level's own)
};

static int mvg_cycle(pmh_mg_mv M, int l, const double *b64, double *z64, bool d0_ready, const int *halt)
{
  pmh_mg       mg = M->mg;
  mg_mv_level &Ml = M->L[l];
  if (l < mg->nlevels - 1) {
    mg_form8 f{mg, M, halt};
    return mg_fused_level(f, l, (const float *)Ml.b, Ml.x, b64, z64, d0_ready);
  }
  hipStream_t st = mg->ctx->stream;
  const dim3  blk(PMH_BLOCK);
  const int   nrep = M->nrep, n_l = mg->L[l].n / nrep; // (congruent blocks: the first block's share of every level)
  const int   nbc = mg->nb_coarse / nrep, ck = mvg_coarse_kind(mg);
  if (ck == MVG_COARSE_MFMA)
    // (16 wavefronts x 2 steps per stage: 21.4 us on the 5 184-row block; 8 x 3: 23.2, 8 x 6: 26.9, 16 x 3: 25.3, 4 x 6: 26.6)
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_mvg_coarse_mfma<16, 2>), dim3(n_l / 16), dim3(64 * 16), 0, st, nbc, halt, (const int *)mg->d_crs, (const long long *)mg->d_cofs,
                       (const _Float16 *)mg->d_cpinv, (float)mg->cp_scale, (const float *)Ml.b, Ml.x);
  else if (ck == MVG_COARSE_F16)
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_mvg_coarse<_Float16>), dim3((n_l + 3) / 4), blk, 0, st, nbc, n_l, halt, (const int *)mg->d_crs,
                       (const long long *)mg->d_cofs, (const _Float16 *)mg->d_cpinv, (float)mg->cp_scale,
                       (const float *)Ml.b, Ml.x);
  else
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_mvg_coarse<float>), dim3((n_l + 3) / 4), blk, 0, st, nbc, n_l, halt, (const int *)mg->d_crs,
                       (const long long *)mg->d_cofs, (const float *)mg->d_cpinv, 1.f, (const float *)Ml.b, Ml.x);
  PMH_HIP(hipGetLastError());
  return PMH_SUCCESS;
}

// Z = V(B) for R columns: b, z are fp64 multivectors of n_0 R entries
int pmh_mg_mv_apply(pmh_mg_mv M, const double *b, double *z, const int *halt)
{
  PMH_ARG(M && b);
  return mvg_cycle(M, 0, b, z, false, halt);
}
const float *pmh_mg_mv_result(pmh_mg_mv M) { return M->L[0].x; }

// ---- test entries (tests/test_gpu_mg_paths.py): the 8-column cycle as an operator -- which kernels it chose, ONE cycle under a halt word of the entry's own, and the work
// multivectors it leaves behind; nothing inside the solvers calls them ----
extern "C" int pmh_mg_mv_test_create(pmh_mg mg, int nrep, void **M_)
{
  PMH_ARG(mg && M_ && nrep >= 1);
  *M_ = nullptr;
  pmh_mg_mv M  = nullptr;
  const int rc = pmh_mg_mv_create(mg, &M, nrep);
  if (rc == PMH_EPI_UNSUPPORTED) return pmh_set_error(PMH_ERR_SUP, "pmh_mg_mv_test_create: %s", pmh_mv_why());
  if (rc) return rc;
  *M_ = M;
  return PMH_SUCCESS;
}

// info = {rows of the level per replica, nrep, transfer kernels to the next level (0 none, 1 node-wise, 2 the rectangular ELL pair, 3 scalar), coarse solve on the last level
// (0 k_mvg_coarse<float>, 1 k_mvg_coarse<_Float16>, 2 matrix cores; -1 on a smoothed level), storage of the level operator's ELL copy (-1 on the last level), the next
// level's d0 rides on the restriction, coarse blocks of one replica, 0}
extern "C" int pmh_mg_mv_test_info(void *M_, int level, long long info[8])
{
  pmh_mg_mv M = (pmh_mg_mv)M_;
  PMH_ARG(M && info && level >= 0 && level < M->mg->nlevels);
  pmh_mg     mg   = M->mg;
  const bool last = level == mg->nlevels - 1;
  info[0] = mg->L[level].n / M->nrep, info[1] = M->nrep, info[2] = mvg_transfer_kind(M, level), info[3] = last ? mvg_coarse_kind(mg) : -1;
  info[4] = last ? -1 : M->L[level].E->storage, info[5] = mg_is_fused_level(mg, level + 1) ? 1 : 0, info[6] = mg->nb_coarse / M->nrep, info[7] = 0;
  return PMH_SUCCESS;
}

// b: fp64 multivector of the fine level (rows of one replica x 8, device); z64: the same for the result, or NULL (the production call: the fp32 result is level 0's x)
extern "C" int pmh_mg_mv_test_apply(void *M_, const double *b, double *z64, int halt)
{
  pmh_mg_mv M = (pmh_mg_mv)M_;
  PMH_ARG(M && b && b != z64);
  pmh_ctx ctx    = M->ctx;
  int    *d_halt = nullptr;
  PMH_CHK(pmh_malloc(ctx, sizeof(int), (void **)&d_halt));
  int rc = pmh_memcpy_h2d(ctx, d_halt, &halt, sizeof(int));
  if (!rc) rc = pmh_mg_mv_apply(M, b, z64, d_halt);
  if (!rc && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = pmh_set_error(PMH_ERR_HIP, "pmh_mg_mv_test_apply: stream synchronisation failed");
  pmh_free(ctx, d_halt);
  return rc;
}

// which: 0 x, 1 b, 2 r, 3 d, 4 t, 5 xa (rows per replica x 8 floats), 6 dinv (rows per replica floats, the hierarchy's own); PMH_ERR_ARG on the last level for 2 .. 6
extern "C" int pmh_mg_mv_test_vector(void *M_, int level, int which, float *host_out)
{
  pmh_mg_mv M = (pmh_mg_mv)M_;
  PMH_ARG(M && host_out && level >= 0 && level < M->mg->nlevels && which >= 0 && which <= 6);
  const mg_mv_level &Ml   = M->L[level];
  const void        *v[7] = {Ml.x, Ml.b, Ml.r, Ml.d, Ml.t, Ml.xa, M->mg->L[level].dinv};
  PMH_ARG(v[which]);
  if (hipStreamSynchronize(M->ctx->stream) != hipSuccess) return pmh_set_error(PMH_ERR_HIP, "pmh_mg_mv_test_vector: stream synchronisation failed");
  const size_t n = (size_t)(M->mg->L[level].n / M->nrep) * (which == 6 ? 1 : MV_R);
  if (n == 0) return PMH_SUCCESS;
  return pmh_memcpy_d2h(M->ctx, host_out, v[which], sizeof(float) * n);
}

extern "C" int pmh_mg_mv_test_destroy(void *M_) { return pmh_mg_mv_destroy((pmh_mg_mv)M_); }
