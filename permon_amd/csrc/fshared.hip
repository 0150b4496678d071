// Explicit local dual operators SHARED by congruent blocks (storage PMH_FX_CLASS of pmh_fexplicit).
//
// Subdomains with bit-identical matrices (pmh_csr_block_classes: the 8 cubes of configs[2], the 64 of configs[3]) have the same K^+,
// so their dense operators W_b = (K^+)[Gamma_b, Gamma_b] are principal sub-matrices of ONE matrix W_c = (K^+)[U_c, U_c] on the union
// U_c of the dofs B touches in any block of the class (the whole boundary of the cube: 33 288 dofs for configs[2]).  Instead of one dense
// matrix per block (8 x 4 n_b^2 = 14.2 GB in symmetric storage) the class keeps W_c once in full (8 n_c^2 = 8.9 GB) and applies it to
// the blocks' vectors TOGETHER: X_c = [xhat_b scattered into U_c]_b is an n_c x 8 multivector (zero where a block does not touch a
// dof), Y_c = W_c X_c ONE pass over the matrix with eight right-hand sides (more blocks than 8: one pass per group of 8).  The matrix
// bytes per F apply drop by 1.6 x for configs[2] (by 2.9 x for the shape of configs[3]); the kernel walks down the rows with the lane
// owning its output columns (no reduction across lanes), and the rows of W_c deal over several GPUs as contiguous ranges.
// The gluing over the multivector numbering (index = (position in U_c) * 8 + slot of the block) is a pmh_gluing, so
//   F lambda = Bc' -> X,  Y = W_c X,  Bc Y (+ all-reduce)           stays three launches.
// Set-up: one K^+ solve per dof of U_c (what the per-block storage already did for congruent blocks), each giving one full row of W_c.
//
// Three storages of W_c live in this file (fx_shared::sym):
//   0  PMH_FX_CLASS        the full matrix, k_fxs_gemm8: 8 n_c^2 bytes per apply, HBM-bound
//   1 PMH_FX_CLASS_SYM its lower block-triangle in 16 x 16 tiles, k_fxs_symm8 (both products of a tile on the fp64 matrix instruction): 4 n_c^2 bytes,
//     HBM-bound
//   2 PMH_FX_CLASS_ORBIT only the rows of the orbit representatives under the class's symmetries, k_fxo_gemm16: a GEMM on the fp64 matrix
//     instruction,
//                          4 n_c^2 / 24 bytes for the cube's 48 operations, compute-bound (the default for congruent cubes)
//     -- and, where all 48 operations of the cube act on one rank, W_c applied in the group's symmetry-adapted basis instead (fshared_adapted.h, orbitbasis.hip):
//     ten small dense blocks, as many bytes read once, memory-bound; knob orbit_adapted
// and the set-up by symmetry (fxs_set_symmetry: one K^+ solve per orbit of rows, self-checked against direct solves) serves 1 and 2.
// The file is split four ways (round 5): fshared_types.h (the storage structures), fshared_kernels.h (the device kernels), fshared_plan.hip (the orbit GEMM's plan, host only)
// and this file: creation, stripes, symmetries, the launches of the products, the assembly by K^+ solves.
#include "fshared_adapted.h"
#include "fx_assemble.h"
#include "orbitbasis.h"

extern char **environ;

static int fxs_build_launch(fx_shared *S)
{
  if (S->sym) {
    // work = (class, group, owned mega band m) one after the other, the longest first, each a run of steps (pairs of column tiles, 128 KB
    // when all four super bands reach that far); the run is cut into one equal share per CU
    struct band { int c, g, m, nj; };
    std::vector<band> bands;
    long long         steps = 0;
    for (int c = 0; c < S->ncls; c++) {
      fxs_class &C = S->C[c];
      for (int m = C.nmb - 1; m >= 0; m--) {
        if (!C.own[FXM_MB * m]) continue;
        for (int g = 0; g < C.ngroups; g++) {
          const int nj = std::min(C.nsb, FXM_MB * (m + 1)) * FXM_RT;
          bands.push_back({c, g, m, nj});
          steps += (nj + 1) / 2;
        }
      }
    }
    int nwg = (int)std::max(1LL, std::min((long long)S->ctx->num_cus, steps));
    if (const char *e = getenv("PMH_FXM_NWG")) nwg = std::max(1, atoi(e));
    std::vector<int>       first(1, 0), items;
    std::vector<long long> iteml;
    std::vector<std::vector<int>> nseg_of(S->ncls);
    for (int c = 0; c < S->ncls; c++) nseg_of[c].assign((size_t)std::max(1, S->C[c].ngroups * S->C[c].nmb), 0);
    {
      long long done = 0; // steps handed out so far
      size_t    bi = 0;
      long long boff = 0; // steps of band bi already handed out
      for (int k = 0; k < nwg; k++) {
        const long long upto = steps * (k + 1) / nwg;
        while (done < upto && bi < bands.size()) {
          const band     &b   = bands[bi];
          const long long bst = (b.nj + 1) / 2, take = std::min(bst - boff, upto - done);
          fxs_class      &C   = S->C[b.c];
          int            &ns  = nseg_of[b.c][(size_t)b.g * C.nmb + b.m];
          items.insert(items.end(), {b.c, b.g, b.m, (int)(2 * boff), (int)std::min<long long>(b.nj, 2 * (boff + take)), ns, 0, 0});
          iteml.push_back(C.woff);
          iteml.push_back(C.ptoff + (long long)b.g * C.ptsize + C.ptm[b.m]);
          ns++, done += take, boff += take;
          if (boff == bst) bi++, boff = 0;
        }
        first.push_back((int)(items.size() / 8));
      }
    }
    int nsegmax = 1;
    S->bytes = 0.0, S->owned_bytes = 0.0;
    for (int c = 0; c < S->ncls; c++) {
      fxs_class &C     = S->C[c];
      double     tiles = 0.0, parts = 0.0;
      std::vector<int> ownm, own_first((size_t)C.nmb + 1, 0);
      C.nseg_max = 0;
      for (int m = 0; m < C.nmb; m++) {
        own_first[m] = (int)ownm.size();
        if (C.own[FXM_MB * m]) ownm.push_back(m);
      }
      C.nown = (int)ownm.size();
      std::vector<long long> ptoff_of((size_t)std::max(1, C.ngroups * C.nown), 0);
      for (int g = 0; g < C.ngroups; g++)
        for (int k = 0; k < C.nown; k++) ptoff_of[(size_t)g * C.nown + k] = C.ptoff + (long long)g * C.ptsize + C.ptm[ownm[k]];
      if (!C.d_ownfirst) PMH_CHK(pmh_malloc(S->ctx, sizeof(int) * own_first.size(), (void **)&C.d_ownfirst));
      PMH_CHK(pmh_memcpy_h2d(S->ctx, C.d_ownfirst, own_first.data(), sizeof(int) * own_first.size()));
      for (int m = 0; m < C.nmb; m++) {
        if (!C.own[FXM_MB * m]) continue;
        const int sb1 = std::min(C.nsb, FXM_MB * (m + 1));
        for (int sb = FXM_MB * m; sb < sb1; sb++) tiles += (double)(sb + 1) * FXM_RT * FXM_RT * 2048.0;
        int ns = 0;
        for (int g = 0; g < C.ngroups; g++) ns = std::max(ns, nseg_of[c][(size_t)g * C.nmb + m]);
        nsegmax = std::max(nsegmax, ns), C.nseg_max = std::max(C.nseg_max, ns);
        // direct sums per item + transposed sums per column
        parts += (double)ns * (sb1 - FXM_MB * m) * FXM_RS * FXS_S * 8.0 + (double)sb1 * FXM_RS * FXS_S * 8.0;
      }
      S->owned_bytes += tiles;
      // the owned tiles once per group + X read (rows + columns) + the partial sums written and read back + Y written
      S->bytes += (double)C.ngroups * (tiles + 2.0 * parts + 2.0 * 8.0 * FXS_S * C.ld);
      if (!C.d_nseg) PMH_CHK(pmh_malloc(S->ctx, sizeof(int) * nseg_of[c].size(), (void **)&C.d_nseg));
      PMH_CHK(pmh_memcpy_h2d(S->ctx, C.d_nseg, nseg_of[c].data(), sizeof(int) * nseg_of[c].size()));
      if (C.d_ptoff) pmh_free(S->ctx, C.d_ptoff), C.d_ptoff = nullptr;
      if (!C.d_ptoff) PMH_CHK(pmh_malloc(S->ctx, sizeof(long long) * ptoff_of.size(), (void **)&C.d_ptoff));
      PMH_CHK(pmh_memcpy_h2d(S->ctx, C.d_ptoff, ptoff_of.data(), sizeof(long long) * ptoff_of.size()));
    }
    S->nwg = items.empty() ? 0 : nwg, S->nseg = nsegmax, S->nitems = (int)(items.size() / 8);
    items.insert(items.end(), {0, 0, 0, 0, 0, 0, 0, 0});
    iteml.insert(iteml.end(), {0, 0});
    if (S->d_wg) pmh_free(S->ctx, S->d_wg);
    if (S->d_items) pmh_free(S->ctx, S->d_items);
    if (S->d_wgl) pmh_free(S->ctx, S->d_wgl);
    PMH_CHK(pmh_malloc(S->ctx, sizeof(int) * first.size(), (void **)&S->d_wg));
    PMH_CHK(pmh_memcpy_h2d(S->ctx, S->d_wg, first.data(), sizeof(int) * first.size()));
    PMH_CHK(pmh_malloc(S->ctx, sizeof(int) * items.size(), (void **)&S->d_items));
    PMH_CHK(pmh_memcpy_h2d(S->ctx, S->d_items, items.data(), sizeof(int) * items.size()));
    PMH_CHK(pmh_malloc(S->ctx, sizeof(long long) * iteml.size(), (void **)&S->d_wgl));
    PMH_CHK(pmh_memcpy_h2d(S->ctx, S->d_wgl, iteml.data(), sizeof(long long) * iteml.size()));
    const long long need = (long long)nsegmax * std::max(16LL, S->nX);
    if (need > S->part_cap) {
      if (S->part) pmh_free(S->ctx, S->part);
      PMH_CHK(pmh_malloc(S->ctx, sizeof(double) * (size_t)need, (void **)&S->part));
      S->part_cap = need;
    }
    return PMH_SUCCESS; // k_fxs_symfin reads only what the items of a mega band wrote
  }
  // segments of the rank's rows: enough of them to give the chip >= ~4000 waves (n_c / 128 column chunks each), at most 32
  int maxrows = 0, chunks = 0;
  for (auto &C : S->C) maxrows = std::max(maxrows, C.r1 - C.r0), chunks += C.ngroups * (C.ld / 128);
  int nseg = std::max(1, std::min(32, (4096 + std::max(1, chunks) - 1) / std::max(1, chunks)));
  nseg     = std::max(1, std::min(nseg, maxrows / FXS_U));
  S->nseg = nseg;
  std::vector<int> wg;
  S->bytes = 0.0;
  for (int c = 0; c < S->ncls; c++) {
    fxs_class &C    = S->C[c];
    const int  rows = C.r1 - C.r0;
    for (int g = 0; g < C.ngroups; g++)
      for (int j = 0; j < nseg; j++) {
        const int lo = C.r0 + (int)((long long)rows * j / nseg), hi = C.r0 + (int)((long long)rows * (j + 1) / nseg);
        for (int c0 = 0; c0 < C.ld; c0 += 512) wg.insert(wg.end(), {c, g, c0, j, lo, hi});
      }
    // its rows once per group + X read + the segment sums written and read back + Y written
    S->bytes += (double)C.ngroups * (8.0 * (double)rows * C.ld + 8.0 * FXS_S * rows + (2.0 * nseg + 1.0) * 8.0 * FXS_S * C.ld);
  }
  S->nwg = (int)(wg.size() / 6);
  wg.insert(wg.end(), {0, 0, 0, 0, 0, 0});
  if (S->d_wg) pmh_free(S->ctx, S->d_wg);
  PMH_CHK(pmh_malloc(S->ctx, sizeof(int) * wg.size(), (void **)&S->d_wg));
  PMH_CHK(pmh_memcpy_h2d(S->ctx, S->d_wg, wg.data(), sizeof(int) * wg.size()));
  const long long need = (long long)nseg * std::max(16LL, S->nX);
  if (need > S->part_cap) {
    if (S->part) pmh_free(S->ctx, S->part);
    PMH_CHK(pmh_malloc(S->ctx, sizeof(double) * (size_t)need, (void **)&S->part));
    S->part_cap = need;
  }
  return pmh_memset(S->ctx, S->part, 0, sizeof(double) * (size_t)need); // column chunks beyond a class's ld / empty segments stay zero
}

// extra_ptr / extra_rel (optional): block-relative dofs ADDED to the touched set of class c (extra_rel[extra_ptr[c] .. extra_ptr[c + 1])): the closure of the
// touched set under the block's symmetry group (pmh_box_symmetry_closure), so that a class whose own touched set is not invariant keeps all its symmetries
int fxs_create(pmh_gluing B, pmh_blockdiag K, const int *block_class, int sym, fx_shared **out, const int *extra_ptr, const int *extra_rel)
{
  PMH_ARG(B && K && block_class && out && B->n_x == K->n);
  pmh_ctx    ctx = B->ctx;
  fx_shared *S   = new fx_shared();
  S->ctx = ctx, S->B = B, S->K = K, S->nb = K->nblocks, S->sym = sym;
  S->cls.assign(block_class, block_class + S->nb);
  S->ncls = 0;
  for (int b = 0; b < S->nb; b++) {
    PMH_ARG(block_class[b] >= 0);
    S->ncls = std::max(S->ncls, block_class[b] + 1);
  }
  S->C.resize(S->ncls);
  std::vector<int> slot(S->nb), group(S->nb);
  for (int b = 0; b < S->nb; b++) {
    fxs_class &C  = S->C[S->cls[b]];
    const int  nl = K->rowstart[b + 1] - K->rowstart[b];
    if (C.blocks.empty()) C.nloc = nl;
    else if (C.nloc != nl) return pmh_set_error(PMH_ERR_ARG, "pmh_fexplicit_create_shared: blocks of class %d differ in size", S->cls[b]);
    slot[b] = (int)C.blocks.size() % FXS_S, group[b] = (int)C.blocks.size() / FXS_S;
    C.blocks.push_back(b);
  }
  if (sym == 2)
    for (auto &C : S->C) {
      C.S = 1;
      while (C.S < FXS_S && C.S < (int)C.blocks.size()) C.S *= 2;
    }
  // union of the touched dofs per class
  for (int c = 0; c < S->ncls; c++) S->C[c].pos.assign((size_t)std::max(1, S->C[c].nloc), -1);
  auto block_of = [&](int i) { return (int)(std::upper_bound(K->rowstart.begin(), K->rowstart.end(), i) - K->rowstart.begin()) - 1; };
  std::vector<int> lb((size_t)std::max(1, B->n_leaves));
  for (int i = 0; i < B->n_leaves; i++) {
    lb[i] = block_of(B->h_row[i]);
    S->C[S->cls[lb[i]]].pos[B->h_row[i] - K->rowstart[lb[i]]] = 0;
  }
  if (extra_ptr && extra_rel)
    for (int c = 0; c < S->ncls; c++)
      for (int e = extra_ptr[c]; e < extra_ptr[c + 1]; e++) {
        if (extra_rel[e] < 0 || extra_rel[e] >= S->C[c].nloc) return pmh_set_error(PMH_ERR_ARG, "pmh_fexplicit_create_shared: extra dof %d of class %d is outside its blocks (%d rows)", extra_rel[e], c, S->C[c].nloc);
        S->C[c].pos[extra_rel[e]] = 0;
      }
  long long wtot = 0, xtot = 0, pttot = 0;
  for (int c = 0; c < S->ncls; c++) {
    fxs_class &C = S->C[c];
    for (int i = 0; i < C.nloc; i++)
      if (C.pos[i] == 0) C.pos[i] = (int)C.urel.size(), C.urel.push_back(i);
    C.nc      = (int)C.urel.size();
    const int pad = sym == 2 ? 32 : (sym ? FXM_RS : FXS_PAD);
    C.ld      = (C.nc + pad - 1) / pad * pad;
    C.ngroups = ((int)C.blocks.size() + FXS_S - 1) / FXS_S;
    C.r0 = 0, C.r1 = C.ld;
    C.woff = wtot, C.xoff = xtot;
    if (sym == 2) {
      if (C.ld == C.nc) C.ld += 32; // a zero row of X behind the touched dofs for the padded k range of the GEMM
    } else if (sym) {
      C.nsb = C.ld / FXM_RS, C.nmb = (C.nsb + FXM_MB - 1) / FXM_MB;
      C.own.assign((size_t)std::max(1, C.nsb), 1);
      C.ptm.assign((size_t)C.nmb + 1, 0);
      for (int m = 0; m < C.nmb; m++) C.ptm[m + 1] = C.ptm[m] + (long long)std::min(C.nsb, FXM_MB * (m + 1)) * FXM_RS * FXS_S;
      C.ptoff = pttot, C.ptsize = C.ptm[C.nmb];
      pttot += C.ngroups * C.ptsize;
      wtot += (long long)FXM_RS * FXM_RS * ((long long)C.nsb * (C.nsb + 1) / 2); // super band sb: (sb + 1) * 16 column tiles x 16 row tiles x 256 doubles
    } else
      wtot += (long long)C.ld * C.ld;
    xtot += (long long)C.ngroups * C.ld * C.S;
    PMH_CHK(pmh_malloc(ctx, sizeof(int) * (size_t)std::max(1, C.nc), (void **)&C.d_urel));
    if (C.nc) PMH_CHK(pmh_memcpy_h2d(ctx, C.d_urel, C.urel.data(), sizeof(int) * (size_t)C.nc));
  }
  if (xtot >= (1LL << 31)) return pmh_set_error(PMH_ERR_SUP, "pmh_fexplicit_create_shared: the multivector numbering exceeds 32-bit indices");
  S->nX = xtot, S->wtot = wtot;
  // gluing over the multivector numbering: leaf of block b at relative dof i -> (position of i in U_c) * 8 + slot(b), group by group
  std::vector<int> rows((size_t)std::max(1, B->n_leaves));
  for (int i = 0; i < B->n_leaves; i++) {
    const int        b = lb[i];
    const fxs_class &C = S->C[S->cls[b]];
    rows[i]            = (int)(C.xoff + (long long)group[b] * C.ld * C.S + (long long)C.pos[B->h_row[i] - K->rowstart[b]] * C.S + slot[b]);
  }
  if (sym == 2) {
    for (auto &C : S->C) C.tmask.assign((size_t)std::max(1, C.ngroups) * std::max(1, C.nc) * FXS_S, 0);
    for (int i = 0; i < B->n_leaves; i++) {
      const int  b = lb[i];
      fxs_class &C = S->C[S->cls[b]];
      C.tmask[((size_t)group[b] * C.nc + C.pos[B->h_row[i] - K->rowstart[b]]) * FXS_S + slot[b]] = 1;
    }
    for (auto &C : S->C) {
      PMH_CHK(pmh_malloc(ctx, C.tmask.size(), (void **)&C.d_tmask));
      PMH_CHK(pmh_memcpy_h2d(ctx, C.d_tmask, C.tmask.data(), C.tmask.size()));
    }
  }
  PMH_CHK(pmh_gluing_create(ctx, (int)std::max(1LL, xtot), B->n_lambda, B->n_leaves, rows.data(), B->h_root.data(), B->h_sign.data(), &S->Bc));
  if (sym == 2) {
    if (2 * xtot >= (1LL << 31)) return pmh_set_error(PMH_ERR_SUP, "pmh_fexplicit_create_shared_orbit: the signed multivector numbering exceeds 32-bit indices");
    std::vector<int>    rows2((size_t)std::max(1, 2 * B->n_leaves)), root2((size_t)std::max(1, 2 * B->n_leaves));
    std::vector<double> sign2((size_t)std::max(1, 2 * B->n_leaves));
    for (int i = 0; i < B->n_leaves; i++) {
      // entry (position, slot) -> (position, +, slot) and (position, -, slot)
      const int slot_i = slot[lb[i]], base = rows[i] - slot_i, Sc = S->C[S->cls[lb[i]]].S;
      rows2[2 * i] = 2 * base + slot_i, rows2[2 * i + 1] = 2 * base + Sc + slot_i;
      root2[2 * i] = root2[2 * i + 1] = B->h_root[i];
      sign2[2 * i] = B->h_sign[i], sign2[2 * i + 1] = -B->h_sign[i];
    }
    PMH_CHK(pmh_gluing_create(ctx, (int)std::max(1LL, 2 * xtot), B->n_lambda, 2 * B->n_leaves, rows2.data(), root2.data(), sign2.data(), &S->Bc2));
    PMH_CHK(pmh_malloc(ctx, sizeof(double) * (size_t)std::max(32LL, 2 * xtot), (void **)&S->X2));
    PMH_CHK(pmh_memset(ctx, S->X2, 0, sizeof(double) * (size_t)std::max(32LL, 2 * xtot)));
  }
  {
    const size_t bytes = sizeof(double) * (size_t)std::max(32LL, wtot);
    hipError_t   e     = hipMalloc((void **)&S->Wbase, bytes);
    if (e != hipSuccess) return pmh_set_error(PMH_ERR_HIP, "pmh_fexplicit_create_shared: %.2f GB for the shared explicit operators: %s", bytes / 1e9, hipGetErrorString(e));
    PMH_HIP(hipMemsetAsync(S->Wbase, 0, bytes, ctx->stream));
  }
  if (sym == 1) {
    S->pt_tot = pttot;
    PMH_CHK(pmh_malloc(ctx, sizeof(double) * (size_t)std::max(16LL, pttot), (void **)&S->pt));
  }
  PMH_CHK(pmh_malloc(ctx, sizeof(double) * (size_t)std::max(16LL, xtot), (void **)&S->X));
  PMH_CHK(pmh_malloc(ctx, sizeof(double) * (size_t)std::max(16LL, xtot), (void **)&S->Y));
  PMH_CHK(pmh_memset(ctx, S->X, 0, sizeof(double) * (size_t)std::max(16LL, xtot)));
  PMH_CHK(pmh_memset(ctx, S->Y, 0, sizeof(double) * (size_t)std::max(16LL, xtot))); // rows of other ranks' stripes stay zero
  std::vector<int>       ldv(S->ncls);
  std::vector<long long> wo(S->ncls), xo(S->ncls);
  for (int c = 0; c < S->ncls; c++) ldv[c] = S->C[c].ld, wo[c] = S->C[c].woff, xo[c] = S->C[c].xoff;
  PMH_CHK(pmh_malloc(ctx, sizeof(int) * S->ncls, (void **)&S->d_ld));
  PMH_CHK(pmh_malloc(ctx, sizeof(long long) * S->ncls, (void **)&S->d_woff));
  PMH_CHK(pmh_malloc(ctx, sizeof(long long) * S->ncls, (void **)&S->d_xoff));
  PMH_CHK(pmh_memcpy_h2d(ctx, S->d_ld, ldv.data(), sizeof(int) * S->ncls));
  PMH_CHK(pmh_memcpy_h2d(ctx, S->d_woff, wo.data(), sizeof(long long) * S->ncls));
  PMH_CHK(pmh_memcpy_h2d(ctx, S->d_xoff, xo.data(), sizeof(long long) * S->ncls));
  if (sym != 2) PMH_CHK(fxs_build_launch(S)); // orbit storage: planned once the symmetries are known (fxo_prepare)
  *out = S;
  return PMH_SUCCESS;
}

static void fxa_free(pmh_ctx ctx, fxs_class &C)
{
  fxa_class *a = C.oa;
  if (!a) return;
  if (a->Wh) (void)hipFree(a->Wh);
  for (void *q : {(void *)a->d_ir, (void *)a->d_tab, (void *)a->Xh, (void *)a->Yh, (void *)a->d_toff, (void *)a->d_osize, (void *)a->d_tbase, (void *)a->d_opos, (void *)a->d_rowinfo, (void *)a->d_items,
                  (void *)a->d_tmask, (void *)a->d_tabN, (void *)a->d_tabNT, (void *)a->d_nfx, (void *)a->d_nyd, (void *)a->d_nxh, (void *)a->d_nyh})
    if (q) pmh_free(ctx, q);
  delete a;
  C.oa = nullptr;
}

void fxs_destroy(fx_shared *S)
{
  if (!S) return;
  pmh_ctx ctx = S->ctx;
  for (auto &C : S->C) {
    if (C.d_urel) pmh_free(ctx, C.d_urel);
    if (C.d_tmask) pmh_free(ctx, C.d_tmask);
    if (C.d_nseg) pmh_free(ctx, C.d_nseg);
    if (C.d_ptoff) pmh_free(ctx, C.d_ptoff);
    if (C.d_ownfirst) pmh_free(ctx, C.d_ownfirst);
    if (C.d_posmap) pmh_free(ctx, C.d_posmap), pmh_free(ctx, C.d_sign);
    if (C.d_gidx) pmh_free(ctx, C.d_gidx), pmh_free(ctx, C.d_reppos), pmh_free(ctx, C.d_use);
    if (C.d_coltab) pmh_free(ctx, C.d_coltab), pmh_free(ctx, C.d_fintab), pmh_free(ctx, C.d_finbase);
    if (C.d_kinv) pmh_free(ctx, C.d_kinv), pmh_free(ctx, C.d_unittab), pmh_free(ctx, C.d_lut);
    fxa_free(ctx, C);
  }
  if (S->pt) pmh_free(ctx, S->pt);
  if (S->d_wgl) pmh_free(ctx, S->d_wgl);
  if (S->d_items) pmh_free(ctx, S->d_items);
  if (S->d_wgfirst) pmh_free(ctx, S->d_wgfirst);
  if (S->d_wgfirst_all) pmh_free(ctx, S->d_wgfirst_all);
  if (S->d_fin_args) pmh_free(ctx, S->d_fin_args);
  if (S->d_zrow_of) pmh_free(ctx, S->d_zrow_of), pmh_free(ctx, (void *)S->d_coltab_of), pmh_free(ctx, (void *)S->d_gidx_of);
  pmh_gluing_destroy(S->Bc);
  for (auto e : S->ev_mid) (void)hipEventDestroy(e);
  pmh_gluing_destroy(S->Bc2);
  pmh_free(ctx, S->X2);
  if (S->Wbase) (void)hipFree(S->Wbase);
  if (S->Afund) (void)hipFree(S->Afund);
  if (S->cpart) pmh_free(ctx, S->cpart);
  if (S->part) pmh_free(ctx, S->part);
  pmh_free(ctx, S->X), pmh_free(ctx, S->Y), pmh_free(ctx, S->d_wg), pmh_free(ctx, S->d_ld), pmh_free(ctx, S->d_woff), pmh_free(ctx, S->d_xoff);
  for (hipEvent_t e : S->ev) (void)hipEventDestroy(e);
  delete S;
}


// the dealing rule of the symmetric tile storage: mega band m of nmb (1024 rows; cost ~ m + 1) -> rank: from the longest down in snake order
static inline int fxm_owner(int m, int nmb, int size)
{
  const int i = nmb - 1 - m, round = i / size, k = i % size;
  return (round & 1) ? size - 1 - k : k;
}

// host helper (no device): the owner rank of every mega band of a class with n_c touched dofs and the tile bytes per rank under that rule
extern "C" int pmh_fexplicit_class_sym_plan(int n_c, int size, int *owner_out, double *bytes_per_rank)
{
  PMH_ARG(n_c >= 1 && size >= 1);
  const int nsb = (n_c + FXM_RS - 1) / FXM_RS, nmb = (nsb + FXM_MB - 1) / FXM_MB;
  if (bytes_per_rank)
    for (int r = 0; r < size; r++) bytes_per_rank[r] = 0.0;
  for (int m = 0; m < nmb; m++) {
    const int o = fxm_owner(m, nmb, size);
    if (owner_out) owner_out[m] = o;
    if (bytes_per_rank)
      for (int sb = FXM_MB * m; sb < std::min(nsb, FXM_MB * (m + 1)); sb++) bytes_per_rank[o] += (double)(sb + 1) * FXM_RT * FXM_RT * 2048.0;
  }
  return PMH_SUCCESS;
}

// several GPUs: rank r applies / assembles the rows [r0, r1) of every W_c, contiguous ranges of equal length (multiples of 32)
int fxs_set_stripe(fx_shared *S, int rank, int size)
{
  if (S->sym == 2) { // orbit storage: a contiguous range of the representatives per rank, planned by fxo_prepare
    S->stripe_rank = rank, S->stripe_size = size, S->fxo_ready = 0;
    return PMH_SUCCESS;
  }
  if (S->sym) {
    // whole mega bands of 1024 rows (a rank assembles exactly the rows it applies); mega band m costs ~ m + 1: dealt from the longest down in
    // snake order, so every rank gets the same number of long and short ones
    for (auto &C : S->C) {
      for (int m = 0; m < C.nmb; m++)
        for (int sb = FXM_MB * m; sb < std::min(C.nsb, FXM_MB * (m + 1)); sb++) C.own[sb] = fxm_owner(m, C.nmb, size) == rank;
    }
    return fxs_build_launch(S);
  }
  for (auto &C : S->C) {
    const int nrg = C.ld / 32; // row groups of 32
    C.r0 = (int)((long long)nrg * rank / size) * 32;
    C.r1 = (int)((long long)nrg * (rank + 1) / size) * 32;
  }
  return fxs_build_launch(S);
}

long long fxs_dense_bytes(fx_shared *S) { return S->sym ? (long long)S->owned_bytes : (long long)sizeof(double) * S->wtot; }
// orbit storage: every class with touched dofs applies W_c in the symmetry-adapted basis (set at the assembly) and the switch is on
static bool fxa_active(fx_shared *S)
{
  if (S->sym != 2 || !pmh_knobs().orbit_adapted) return false;
  bool any = false;
  for (const fxs_class &C : S->C) {
    if (!C.nc) continue;
    if (!C.oa) return false;
    any = true;
  }
  return any;
}
int fxs_orbit_adapted(fx_shared *S, int c) { return c >= 0 && c < S->ncls && S->C[c].oa && fxa_active(S); }
// orbit storage: the GEMM's useful flops per apply; in the symmetry-adapted basis what the blocks' products and the two transforms need / execute
double fxs_apply_flops(fx_shared *S)
{
  if (!fxa_active(S)) return S->sym == 2 ? S->flops : 0.0;
  double f = 0.0;
  for (const fxs_class &C : S->C)
    if (C.oa) f += C.oa->flops;
  return f;
}
void fxs_apply_flops_detail(fx_shared *S, double *issued, double *dense)
{
  *issued = S->sym == 2 ? S->flops_issued : 0.0, *dense = S->sym == 2 ? S->flops_dense : 0.0;
  if (!fxa_active(S)) return;
  *issued = 0.0;
  for (const fxs_class &C : S->C)
    if (C.oa) *issued += C.oa->flops_issued;
}
double fxs_apply_bytes(fx_shared *S)
{
  if (!fxa_active(S)) return S->bytes;
  double b = 0.0;
  for (const fxs_class &C : S->C)
    if (C.oa) b += C.oa->bytes;
  return b;
}

// the touched dofs of class c, ascending, relative to the block start (the numbering of W_c's rows)
int fxs_class_union(fx_shared *S, int c, int *n_c, int *urel_out)
{
  PMH_ARG(S && c >= 0 && c < S->ncls);
  if (n_c) *n_c = S->C[c].nc;
  if (urel_out && S->C[c].nc) memcpy(urel_out, S->C[c].urel.data(), sizeof(int) * (size_t)S->C[c].nc);
  return PMH_SUCCESS;
}

// Set-up by symmetry: nsym signed permutations of U_c (posmap[g * n_c + c] = position of the image of the c-th touched dof, sign = +-1; operation 0 the
// identity) under which K_c, hence K_c^+, is invariant: W[g p][g c] = sign_g[p] sign_g[c] W[p][c], so ONE K^+ solve serves the whole orbit of a row
// (a cube of Q1 elasticity elements: the 48 signed coordinate permutations -> 48 x fewer solves).  The caller vouches for the invariance (permon_amd
// checks the generators against K); the assembly re-solves a handful of symmetry-filled rows directly and fails if they differ.
int fxs_set_symmetry(fx_shared *S, int c, int nsym, const int *posmap, const signed char *sign)
{
  PMH_ARG(S && c >= 0 && c < S->ncls && nsym >= 1 && posmap && sign);
  if (!S->sym) return pmh_set_error(PMH_ERR_SUP, "pmh_fexplicit_set_class_symmetry: needs the PMH_FX_CLASS_SYM or PMH_FX_CLASS_ORBIT storage");
  S->fxo_ready = 0;
  fxs_class &C  = S->C[c];
  const int  nc = C.nc;
  std::vector<char> seen((size_t)std::max(1, nc));
  for (int g = 0; g < nsym; g++) {
    std::fill(seen.begin(), seen.end(), 0);
    for (int i = 0; i < nc; i++) {
      const int t = posmap[(size_t)g * nc + i];
      if (t < 0 || t >= nc || seen[t] || (sign[(size_t)g * nc + i] != 1 && sign[(size_t)g * nc + i] != -1))
        return pmh_set_error(PMH_ERR_ARG, "pmh_fexplicit_set_class_symmetry: operation %d is not a signed permutation of the %d touched dofs", g, nc);
      if (g == 0 && (t != i || sign[i] != 1)) return pmh_set_error(PMH_ERR_ARG, "pmh_fexplicit_set_class_symmetry: operation 0 must be the identity");
      seen[t] = 1;
    }
  }
  C.nsym = nsym;
  C.h_ops.clear(); // (set-up by box symmetries hands them on afterwards: fxs_set_symmetry_ops)
  fxa_free(S->ctx, C);
  C.h_posmap.assign(posmap, posmap + (size_t)nsym * nc);
  C.h_sign.assign(sign, sign + (size_t)nsym * nc);
  if (C.d_posmap) pmh_free(S->ctx, C.d_posmap), pmh_free(S->ctx, C.d_sign);
  PMH_CHK(pmh_malloc(S->ctx, sizeof(int) * (size_t)std::max(1, nsym * nc), (void **)&C.d_posmap));
  PMH_CHK(pmh_malloc(S->ctx, (size_t)std::max(1, nsym * nc), (void **)&C.d_sign));
  if (nc) {
    PMH_CHK(pmh_memcpy_h2d(S->ctx, C.d_posmap, C.h_posmap.data(), sizeof(int) * (size_t)nsym * nc));
    PMH_CHK(pmh_memcpy_h2d(S->ctx, C.d_sign, C.h_sign.data(), (size_t)nsym * nc));
  }
  return PMH_SUCCESS;
}


int fxs_set_symmetry_ops(fx_shared *S, int c, int nsym, const int *ops)
{
  PMH_ARG(S && c >= 0 && c < S->ncls && ops && nsym == S->C[c].nsym);
  S->C[c].h_ops.assign(ops, ops + 6 * (size_t)nsym);
  return PMH_SUCCESS;
}

// The k_fxo_gemm16 instantiation of a row tile tm, a column tile tn (128 / 64) and tnw (48: one-block classes): 1000 + tm for the single-class kernel (tn = 128), tm + 1 for
// tn = 64 and one more for tnw = 48 on the table-driven (MULTI) kernels; 0: no such kernel.  The launches below and pmh_fexplicit_orbit_plan_info go by it.
static int fxo_instance(int tm, int tn, int tnw, bool tables)
{
  if (tnw == 48) return tables && tn == 64 && (tm == 192 || tm == 128 || tm == 64) ? tm + 2 : 0;
  if (tm != 144 && tm != 128 && tm != 112 && tm != 96 && tm != 80) return 0;
  if (!tables) return tn == 128 ? 1000 + tm : 0;
  return tn == 64 ? tm + 1 : (tn == 128 ? tm : 0);
}
// how class c is launched: 2 in the ONE launch over all classes' items (merged), 1 by a table-driven launch of its own (records of fewer than 8 slots), 0 by the single-class kernel
static int fxo_launch_kind(const fx_shared *S, const fxs_class &C) { return S->merged_tm > 0 && S->nwg_all > 0 ? 2 : (C.S != FXS_S ? 1 : 0); }

static int fxo_gemm(fx_shared *S)
{
  hipStream_t st = S->ctx->stream;
  // several classes on one row tile: one GEMM launch over all their items, then the classes' finishing launches
  const bool  merged = S->merged_tm > 0 && S->nwg_all > 0;
  if (merged) {
#define FXO_LAUNCH_ALL(NI, NWM, TNW)                                                                                                                                                                      \
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fxo_gemm16<NI, NWM, true, TNW>), dim3(S->nwg_all), dim3(256), 0, st, (const int *)S->d_items, (const long long *)S->d_wgl, (const int *)S->d_wg,                 \
                     (const int *)(S->d_wg + S->ncls), (const int *)nullptr, 0, (const double *)S->Afund, (const int *)nullptr, (const double *)S->X2, S->cpart, (const int *)S->d_wgfirst_all, \
                     (const int *const *)S->d_coltab_of, (const int *)S->d_zrow_of, (const int *const *)S->d_gidx_of, (const int *)(S->d_zrow_of + S->ncls))
    switch (fxo_instance(S->merged_tm, S->merged_tn, S->merged_tnw, true)) {
    case 194: FXO_LAUNCH_ALL(3, 4, 48); break;
    case 130: FXO_LAUNCH_ALL(2, 4, 48); break;
    case 66: FXO_LAUNCH_ALL(1, 4, 48); break;
    case 144: FXO_LAUNCH_ALL(9, 1, 128); break;
    case 145: FXO_LAUNCH_ALL(9, 1, 64); break;
    case 128: FXO_LAUNCH_ALL(4, 2, 128); break;
    case 129: FXO_LAUNCH_ALL(4, 2, 64); break;
    case 112: FXO_LAUNCH_ALL(7, 1, 128); break;
    case 113: FXO_LAUNCH_ALL(7, 1, 64); break;
    case 96: FXO_LAUNCH_ALL(3, 2, 128); break;
    case 97: FXO_LAUNCH_ALL(3, 2, 64); break;
    case 80: FXO_LAUNCH_ALL(5, 1, 128); break;
    case 81: FXO_LAUNCH_ALL(5, 1, 64); break;
    default: return pmh_set_error(PMH_ERR_STATE, "PMH_FX_CLASS_ORBIT: row tile %d has no 16x16x4 kernel", S->merged_tm);
    }
#undef FXO_LAUNCH_ALL
    if (S->ev_mid_pending >= 0) PMH_HIP(hipEventRecord(S->ev_mid[S->ev_mid_pending], st));
  }
  for (int c = 0; c < S->ncls; c++) { // one launch per class (its own gather-index array and column lists); configs[2] / [3]: one class
    fxs_class &C = S->C[c];
    if (!C.nc) continue;
    const int first = C.item_first, count = C.wg_count; // the class's items are contiguous
    if (!count) continue;
#define FXO_LAUNCH(KERNEL)                                                                                                                                                                              \
  hipLaunchKernelGGL(KERNEL, dim3(count), dim3(256), 0, st, (const int *)(S->d_items + 8 * first), (const long long *)(S->d_wgl + 4 * first), (const int *)S->d_wg, (const int *)(S->d_wg + S->ncls), \
                     (const int *)C.d_coltab, C.nsymp, (const double *)S->Afund, (const int *)C.d_gidx, (const double *)S->X2, S->cpart, (const int *)(S->d_wgfirst + C.wgf_first))
#ifdef FXO_TRACE
    static unsigned long long *d_trace = nullptr;
    static int                 traced  = 0;
    if (!d_trace) {
      PMH_HIP(hipMalloc((void **)&d_trace, sizeof(unsigned long long) * 8 * 64 * 8));
      PMH_HIP(hipMemcpyToSymbol(HIP_SYMBOL(fxo_trace_buf), &d_trace, sizeof(d_trace)));
    }
    PMH_HIP(hipMemsetAsync(d_trace, 0, sizeof(unsigned long long) * 8 * 64 * 8, st));
#endif
    if (merged) {
      // (the class's products were part of the launch above)
    } else if (fxo_launch_kind(S, C) == 1) { // records of fewer than 8 slots: the table-driven kernel on this class's slice of the items
#define FXO_LAUNCH_T(NI, NWM, TNW)                                                                                                                                                                             \
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fxo_gemm16<NI, NWM, true, TNW>), dim3(count), dim3(256), 0, st, (const int *)(S->d_items + 8 * first), (const long long *)(S->d_wgl + 4 * first), (const int *)S->d_wg, \
                     (const int *)(S->d_wg + S->ncls), (const int *)nullptr, 0, (const double *)S->Afund, (const int *)nullptr, (const double *)S->X2, S->cpart, (const int *)(S->d_wgfirst + C.wgf_first),     \
                     (const int *const *)S->d_coltab_of, (const int *)S->d_zrow_of, (const int *const *)S->d_gidx_of, (const int *)(S->d_zrow_of + S->ncls))
      switch (fxo_instance(C.tm, C.tn, C.tnw, true)) {
      case 194: FXO_LAUNCH_T(3, 4, 48); break;
      case 130: FXO_LAUNCH_T(2, 4, 48); break;
      case 66: FXO_LAUNCH_T(1, 4, 48); break;
      case 144: FXO_LAUNCH_T(9, 1, 128); break;
      case 145: FXO_LAUNCH_T(9, 1, 64); break;
      case 128: FXO_LAUNCH_T(4, 2, 128); break;
      case 129: FXO_LAUNCH_T(4, 2, 64); break;
      case 112: FXO_LAUNCH_T(7, 1, 128); break;
      case 113: FXO_LAUNCH_T(7, 1, 64); break;
      case 96: FXO_LAUNCH_T(3, 2, 128); break;
      case 97: FXO_LAUNCH_T(3, 2, 64); break;
      case 80: FXO_LAUNCH_T(5, 1, 128); break;
      case 81: FXO_LAUNCH_T(5, 1, 64); break;
      default: return pmh_set_error(PMH_ERR_STATE, "PMH_FX_CLASS_ORBIT: row tile %d has no 16x16x4 kernel", C.tm);
      }
#undef FXO_LAUNCH_T
    } else {
      switch (fxo_instance(C.tm, C.tn, C.tnw, false)) {
      case 1144: FXO_LAUNCH((k_fxo_gemm16<9, 1>)); break;
      case 1128: FXO_LAUNCH((k_fxo_gemm16<4, 2>)); break;
      case 1112: FXO_LAUNCH((k_fxo_gemm16<7, 1>)); break;
      case 1096: FXO_LAUNCH((k_fxo_gemm16<3, 2>)); break;
      case 1080: FXO_LAUNCH((k_fxo_gemm16<5, 1>)); break;
      default: return pmh_set_error(PMH_ERR_STATE, "PMH_FX_CLASS_ORBIT: row tile %d has no 16x16x4 kernel", C.tm);
      }
    }
#undef FXO_LAUNCH
    // (one class: configs[2] / [3]; several classes: after the last class's GEMM)
    if (!merged && S->ev_mid_pending >= 0 && c == S->ncls - 1) PMH_HIP(hipEventRecord(S->ev_mid[S->ev_mid_pending], st));
#ifdef FXO_TRACE
    if (++traced == 300) { // one launch in the steady state of the bench
      std::vector<unsigned long long> h(8 * 64 * 8);
      PMH_HIP(hipStreamSynchronize(st));
      PMH_HIP(hipMemcpy(h.data(), d_trace, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost));
      for (int w = 0; w < 8; w++) {
        fprintf(stderr, "FXO_TRACE workgroup %d (cycles of the shader clock; per chunk: loads issued | products | wait vmcnt | LDS store | barrier | total)\n", w * 37);
        for (int ch = 0; ch < 63; ch++) {
          const unsigned long long *q = &h[((size_t)w * 64 + ch) * 8];
          if (!q[5]) break;
#ifdef FXO_TRACE_FULL
          fprintf(stderr, "  chunk %2d: %6llu | %6llu | %6llu | %6llu | %6llu | %6llu\n", ch, q[1] - q[0], q[2] - q[1], q[3] - q[2], q[4] - q[3], q[5] - q[4], q[5] - q[0]);
#else
          // loads + products | store + barrier
          fprintf(stderr, "  chunk %2d: %6llu | %6llu | %6llu | %6llu | %6llu | %6llu\n", ch, 0ULL, q[2] - q[0], 0ULL, 0ULL, q[5] - q[2], q[5] - q[0]);
#endif
        }
      }
    }
#endif
    if (C.fin_elems > 0 && !S->d_fin_args)
      hipLaunchKernelGGL(k_fxo_fin, dim3((unsigned)((C.fin_elems + PMH_BLOCK - 1) / PMH_BLOCK), C.ngroups), dim3(PMH_BLOCK), 0, st, C.Mp / C.tm, C.tm, C.nsymp, C.nc, (const int *)C.d_fintab,
                         (const int *)C.d_unittab, (const long long *)C.d_finbase, (const int *)C.d_lut, (const int *)C.d_coltab, (const double *)S->cpart, (const signed char *)C.d_use, (const int *)C.d_reppos, (const int *)C.d_posmap, C.xoff, C.ld,
                         S->Y, C.S, (const char *)C.d_tmask);
  }
  if (S->d_fin_args && S->fin_nbx > 0) // after ALL classes' products
    hipLaunchKernelGGL(k_fxo_fin_all, dim3((unsigned)S->fin_nbx, (unsigned)S->fin_ngroups, (unsigned)S->ncls), dim3(PMH_BLOCK), 0, st, (const fxo_fin_args *)S->d_fin_args, (const double *)S->cpart, S->Y);
  PMH_HIP(hipGetLastError());
  return PMH_SUCCESS;
}

// X (position, slot) -> X2 (position, +-, slot): only for the dense kernel alone on a multivector handed in (pmh_fexplicit_dense_mult); the operator fills X2
// by its own gluing
__global__ __launch_bounds__(PMH_BLOCK) void k_fxo_signed_copy(long long n, int nslot, const double *__restrict__ X, double *__restrict__ X2)
{
  for (long long i = (long long)blockIdx.x * PMH_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * PMH_BLOCK) {
    const long long p = i / nslot, sl = i % nslot;
    const double    v = X[i];
    X2[2 * p * nslot + sl] = v, X2[(2 * p + 1) * nslot + sl] = -v;
  }
}

// ---- orbit storage applied in the symmetry-adapted basis (kernels: fshared_adapted.h, basis: orbitbasis.hip) ---------------------------------------------------
// forward transform, the ten blocks' products, inverse transform; the mid event (fxs_timing_get: first_kernel_ms) is recorded before the last launch
// one class's transform, X^ = U' X (inv = false) or Y = U Y^: k_fxa_narrow where the set-up chose it (fxa_class::narrow), k_fxa_transform otherwise
static void fxa_launch_transform(fx_shared *S, const fxs_class &C, bool inv)
{
  const fxa_class *a  = C.oa;
  hipStream_t      st = S->ctx->stream;
  if (a->narrow) {
    const dim3 grid(a->norb, C.ngroups), block(FXN_T);
    if (inv)
      hipLaunchKernelGGL(k_fxa_narrow<true>, grid, block, 0, st, (const double *)a->d_tabNT, (const int *)a->d_osize, (const int *)a->d_nyd, (const long long *)a->d_nyh, a->norb, (long long)C.ld * FXS_S,
                         (const double *)a->Yh, S->Y + C.xoff);
    else
      hipLaunchKernelGGL(k_fxa_narrow<false>, grid, block, 0, st, (const double *)a->d_tabN, (const int *)a->d_osize, (const int *)a->d_nfx, (const long long *)a->d_nxh, a->norb, 2LL * C.ld * FXS_S,
                         (const double *)(S->X2 + 2 * C.xoff), a->Xh);
    return;
  }
  const dim3 grid(a->norb, (a->NC + FXA_CB - 1) / FXA_CB);
  if (inv)
    hipLaunchKernelGGL(k_fxa_transform<true>, grid, dim3(PMH_BLOCK), 0, st, (const fxa_irrep *)a->d_ir, (const double *)a->d_tab, (const long long *)a->d_toff, (const int *)a->d_osize, (const int *)a->d_tbase,
                       (const int *)a->d_opos, (const int *)a->d_rowinfo, a->NC, C.nc, C.ld, C.xoff, (const double *)S->X2, a->Xh, (const double *)a->Yh, S->Y, (const char *)a->d_tmask);
  else
    hipLaunchKernelGGL(k_fxa_transform<false>, grid, dim3(PMH_BLOCK), 0, st, (const fxa_irrep *)a->d_ir, (const double *)a->d_tab, (const long long *)a->d_toff, (const int *)a->d_osize, (const int *)a->d_tbase,
                       (const int *)a->d_opos, (const int *)a->d_rowinfo, a->NC, C.nc, C.ld, C.xoff, (const double *)S->X2, a->Xh, (const double *)a->Yh, S->Y, (const char *)a->d_tmask);
}

static int fxa_launch(fx_shared *S)
{
  hipStream_t st = S->ctx->stream;
  for (fxs_class &C : S->C)
    if (C.oa) fxa_launch_transform(S, C, false);
  for (fxs_class &C : S->C)
    if (fxa_class *a = C.oa)
      if (a->nitems) hipLaunchKernelGGL(k_fxa_prod, dim3(a->nitems), dim3(64 * FXA_WAVES), 0, st, (const int *)a->d_items, (const fxa_irrep *)a->d_ir, (const double *)a->Wh, (const double *)a->Xh, a->Yh);
  if (S->ev_mid_pending >= 0) PMH_HIP(hipEventRecord(S->ev_mid[S->ev_mid_pending], st));
  for (fxs_class &C : S->C)
    if (C.oa) fxa_launch_transform(S, C, true);
  PMH_HIP(hipGetLastError());
  return PMH_SUCCESS;
}

template <class T> static int fxa_upload(pmh_ctx ctx, const std::vector<T> &h, T **d)
{
  PMH_CHK(pmh_malloc(ctx, sizeof(T) * std::max<size_t>(1, h.size()), (void **)d));
  if (!h.empty()) PMH_CHK(pmh_memcpy_h2d(ctx, *d, h.data(), sizeof(T) * h.size()));
  return PMH_SUCCESS;
}

// the class's basis, its device tables and the blocks W^_i from the representatives' rows of A (after fxs_assemble has filled them); a class whose operations
// give no such basis keeps the GEMM (C.oa stays null)
static int fxa_build_class(fx_shared *S, fxs_class &C, bool spoil)
{
  pmh_ctx     ctx = S->ctx;
  oab_basis   B;
  std::string why;
  if (!oab_build(C.nsym, C.nc, C.h_posmap.data(), C.h_sign.data(), C.h_ops.data(), B, why)) {
    if (getenv("PMH_ORBIT_ADAPTED_VERBOSE")) fprintf(stderr, "orbit_adapted: no basis (%s): the class keeps the GEMM\n", why.c_str());
    return PMH_SUCCESS;
  }
  if (B.norb != C.M_all) return PMH_SUCCESS;
  for (int o = 0; o < B.norb; o++) // orbit o's representative is row reprow[o] of A (fxo_prepare numbers the orbits the same way)
    if (B.opos[B.tbase[o]] != C.reps[o]) return PMH_SUCCESS;
  fxa_class *a = new fxa_class();
  C.oa = a;
  a->norb = B.norb, a->NC = C.ngroups * FXS_S, a->nc = C.nc;
  const int M = C.M_all;
  long long wtot = 0, htot = 0, ytot = 0;
  // the one place that chooses the transforms' kernels: k_fxa_narrow for one or two groups of columns (the record of the inverse direction packs the position into 24 bits)
  a->narrow = pmh_knobs().orbit_narrow && a->NC <= FXN_NC && C.nc < (1 << 23);
  double    tfl = 0.0, tfl_issued = 0.0, tab_read = 0.0;
  for (int o = 0; o < B.norb; o++) {
    const double no = B.osize[o], no4 = (B.osize[o] + 3) & ~3;
    tfl += 2.0 * 2.0 * no * no * a->NC;
    tfl_issued += 2.0 * 2.0 * no * (a->narrow ? no4 : no) * a->NC;
    tab_read += a->narrow ? no * no4 * C.ngroups : 48.0 * 48.0; // the rows its threads read per (orbit, group) / the whole table
  }
  a->flops = tfl, a->flops_issued = tfl_issued;
  for (int i = 0; i < OAB_NIRREP; i++) {
    fxa_irrep &I = a->ir[i];
    I.d = B.d[i], I.m = B.m[i];
    I.nks = ((I.m + 7) / 8 + FXA_KU - 1) / FXA_KU * FXA_KU, I.nob = (I.m + 15) / 16, I.nbt = (I.d * a->NC + 15) / 16, I.ldy = 16 * I.nbt;
    I.woff = wtot, I.hoff = htot, I.yoff = ytot;
    wtot += (long long)I.nob * I.nks * 128, htot += (long long)I.nbt * I.nks * 128, ytot += (long long)I.nob * 16 * I.ldy;
    a->flops += 2.0 * (double)I.m * I.m * I.d * a->NC;
    a->flops_issued += 2.0 * (16.0 * I.nob) * (8.0 * I.nks) * (16.0 * I.nbt);
  }
  // the blocks once, X^ written and read, Y^ written and read, a table copy per transform, X read and Y written; the narrow transforms' records (12 bytes per function and group, twice)
  a->bytes = 8.0 * ((double)wtot + 2.0 * htot + 2.0 * ytot + 2.0 * tab_read + 2.0 * (double)C.nc * a->NC) + (a->narrow ? 2.0 * 12.0 * C.nc * C.ngroups : 0.0);
  {
    const size_t bytes = sizeof(double) * (size_t)std::max(128LL, wtot);
    hipError_t   e     = hipMalloc((void **)&a->Wh, bytes);
    if (e != hipSuccess) return pmh_set_error(PMH_ERR_HIP, "PMH_FX_CLASS_ORBIT: %.2f GB for the blocks of the symmetry-adapted form: %s", bytes / 1e9, hipGetErrorString(e));
    PMH_HIP(hipMemsetAsync(a->Wh, 0, bytes, ctx->stream));
  }
  PMH_CHK(pmh_malloc(ctx, sizeof(double) * (size_t)std::max(128LL, htot), (void **)&a->Xh));
  PMH_CHK(pmh_malloc(ctx, sizeof(double) * (size_t)std::max(128LL, ytot), (void **)&a->Yh));
  PMH_CHK(pmh_memset(ctx, a->Xh, 0, sizeof(double) * (size_t)std::max(128LL, htot))); // rows past m and columns past D stay zero
  PMH_CHK(pmh_memset(ctx, a->Yh, 0, sizeof(double) * (size_t)std::max(128LL, ytot)));
  std::vector<int> rowinfo((size_t)C.nc), orb_of((size_t)C.nc), items;
  for (int o = 0; o < B.norb; o++)
    for (int t = 0; t < B.osize[o]; t++) orb_of[B.tbase[o] + t] = o;
  for (int r = 0; r < C.nc; r++) rowinfo[r] = B.row_irrep[r] | (B.row_partner[r] << 4) | (B.row_index[r] << 8);
  { // the longest irreps first
    int order[OAB_NIRREP];
    for (int i = 0; i < OAB_NIRREP; i++) order[i] = i;
    std::stable_sort(order, order + OAB_NIRREP, [&](int x, int y) { return a->ir[x].m > a->ir[y].m; });
    for (int i : order) {
      const fxa_irrep &I = a->ir[i];
      for (int nb0 = 0; nb0 < I.nbt; nb0 += 4)
        for (int ob = 0; ob < I.nob; ob++) {
          const int nbw = std::min(4, I.nbt - nb0);
          items.insert(items.end(), {i, ob, nb0, nbw});
          a->items_of_width[i][nbw - 1]++;
        }
    }
    a->nitems = (int)(items.size() / 4);
  }
  std::vector<fxa_irrep> irv(a->ir, a->ir + OAB_NIRREP);
  std::vector<char>      tmask(C.tmask.begin(), C.tmask.end());
  PMH_CHK(fxa_upload(ctx, irv, &a->d_ir));
  std::vector<double>    tabp((size_t)B.norb * 48 * 48, 0.0); // every table as 48 x 48
  std::vector<long long> toffp((size_t)B.norb);
  for (int o = 0; o < B.norb; o++) {
    toffp[o] = (long long)o * 48 * 48;
    for (int t = 0; t < B.osize[o]; t++)
      for (int j = 0; j < B.osize[o]; j++) tabp[(size_t)toffp[o] + t * 48 + j] = B.tab[(size_t)B.toff[o] + (size_t)t * B.osize[o] + j];
  }
  PMH_CHK(fxa_upload(ctx, tabp, &a->d_tab));
  PMH_CHK(fxa_upload(ctx, toffp, &a->d_toff));
  PMH_CHK(fxa_upload(ctx, B.osize, &a->d_osize));
  PMH_CHK(fxa_upload(ctx, B.tbase, &a->d_tbase));
  PMH_CHK(fxa_upload(ctx, B.opos, &a->d_opos));
  PMH_CHK(fxa_upload(ctx, rowinfo, &a->d_rowinfo));
  PMH_CHK(fxa_upload(ctx, items, &a->d_items));
  PMH_CHK(fxa_upload(ctx, tmask, &a->d_tmask));
  if (a->narrow) { // k_fxa_narrow's records (their layout: fshared_adapted.h); an orbit's functions past its size are never read
    const size_t     nf = (size_t)C.ngroups * B.norb * 48;
    std::vector<int> nfx((size_t)B.norb * 48, 0), nyd(nf, 0);
    std::vector<long long> nxh(nf, 0), nyh(nf, 0);
    for (int o = 0; o < B.norb; o++)
      for (int t = 0; t < B.osize[o]; t++) {
        const int        r = B.tbase[o] + t, pos = B.opos[r];
        const fxa_irrep &I = a->ir[B.row_irrep[r]];
        nfx[(size_t)o * 48 + t] = 2 * FXS_S * pos;
        for (int g = 0; g < C.ngroups; g++) {
          const size_t f = ((size_t)g * B.norb + o) * 48 + t;
          const int    n = B.row_partner[r] * a->NC + FXS_S * g; // the group's slot 0
          int          bits = 0;
          for (int sl = 0; sl < FXS_S; sl++) bits |= (C.tmask[((size_t)g * C.nc + pos) * FXS_S + sl] ? 1 : 0) << sl;
          nxh[f] = fxa_xh_off(I, B.row_index[r], n), nyh[f] = I.yoff + (long long)B.row_index[r] * I.ldy + n, nyd[f] = pos << 8 | bits;
        }
      }
    PMH_CHK(fxa_upload(ctx, nfx, &a->d_nfx));
    PMH_CHK(fxa_upload(ctx, nyd, &a->d_nyd));
    PMH_CHK(fxa_upload(ctx, nxh, &a->d_nxh));
    PMH_CHK(fxa_upload(ctx, nyh, &a->d_nyh));
  }
  // the blocks: the forward transform of the representatives' rows, then the d-term combination per entry
  double *Abuf = nullptr;
  int    *d_reprow = nullptr;
  PMH_CHK(pmh_malloc(ctx, sizeof(double) * (size_t)C.nc * M, (void **)&Abuf));
  PMH_CHK(fxa_upload(ctx, C.reprow, &d_reprow));
  { // step 0: the rows of representatives with a stabiliser, averaged over it
    std::vector<int> hops;
    int             *d_hops = nullptr;
    double          *tmp = nullptr;
    PMH_CHK(pmh_malloc(ctx, sizeof(int) * OAB_NOP, (void **)&d_hops));
    PMH_CHK(pmh_malloc(ctx, sizeof(double) * (size_t)C.nc, (void **)&tmp));
    const int nbx = std::max(1, std::min(64, (C.nc + PMH_BLOCK - 1) / PMH_BLOCK));
    for (int o = 0; o < B.norb; o++) {
      if (B.osize[o] == OAB_NOP) continue;
      const int p = C.reps[o];
      hops.clear();
      for (int g = 0; g < OAB_NOP; g++)
        if (C.h_posmap[(size_t)g * C.nc + p] == p) hops.push_back(g);
      PMH_CHK(pmh_memcpy_h2d(ctx, d_hops, hops.data(), sizeof(int) * hops.size())); // (synchronous: the buffer is free again)
      hipLaunchKernelGGL(k_fxa_stab_avg, dim3(nbx), dim3(PMH_BLOCK), 0, ctx->stream, (int)hops.size(), (const int *)d_hops, p, C.reprow[o], C.tm, C.nc, C.nkc, (const int *)C.d_posmap, (const signed char *)C.d_sign,
                         (const int *)C.d_kinv, (const double *)(S->Afund + C.aoff), tmp);
      hipLaunchKernelGGL(k_fxa_stab_store, dim3(nbx), dim3(PMH_BLOCK), 0, ctx->stream, C.reprow[o], C.tm, C.nc, C.nkc, (const int *)C.d_kinv, (const double *)tmp, S->Afund + C.aoff);
      PMH_CHK(pmh_sync(ctx));
    }
    pmh_free(ctx, d_hops), pmh_free(ctx, tmp);
  }
  hipLaunchKernelGGL(k_fxa_rows, dim3(B.norb, (M + 63) / 64), dim3(64), 0, ctx->stream, M, C.tm, C.nkc, (const double *)a->d_tab, (const long long *)a->d_toff, (const int *)a->d_osize, (const int *)a->d_tbase,
                     (const int *)a->d_opos, (const int *)C.d_kinv, (const int *)d_reprow, (const double *)(S->Afund + C.aoff), Abuf);
  int rc = PMH_SUCCESS;
  for (int i = 0; i < OAB_NIRREP && !rc; i++) {
    const fxa_irrep &I = a->ir[i];
    if (!I.m) continue;
    std::vector<int>    fn0((size_t)I.m), orb((size_t)I.m);
    std::vector<double> vs(3 * (size_t)I.m);
    for (int r = 0; r < C.nc; r++)
      if (B.row_irrep[r] == i && B.row_partner[r] == 0) {
        const int k = B.row_index[r], o = orb_of[r];
        fn0[k] = r, orb[k] = o;
        for (int b = 0; b < 3; b++) vs[3 * (size_t)k + b] = B.row_vs[3 * (size_t)r + b];
      }
    int    *d_fn0 = nullptr, *d_orb = nullptr;
    double *d_vs = nullptr;
    if ((rc = fxa_upload(ctx, fn0, &d_fn0)) || (rc = fxa_upload(ctx, orb, &d_orb)) || (rc = fxa_upload(ctx, vs, &d_vs))) break;
    hipLaunchKernelGGL(k_fxa_combine, dim3((unsigned)(((long long)I.m * I.m + PMH_BLOCK - 1) / PMH_BLOCK)), dim3(PMH_BLOCK), 0, ctx->stream, I, M, (const int *)d_fn0, (const int *)d_orb, (const double *)d_vs,
                       (const double *)Abuf, a->Wh);
    rc = pmh_sync(ctx);
    pmh_free(ctx, d_fn0), pmh_free(ctx, d_orb), pmh_free(ctx, d_vs);
  }
  if (!rc) rc = pmh_sync(ctx);
  pmh_free(ctx, Abuf), pmh_free(ctx, d_reprow);
  if (!rc && hipGetLastError() != hipSuccess) rc = pmh_set_error(PMH_ERR_HIP, "PMH_FX_CLASS_ORBIT: a set-up launch of the symmetry-adapted form failed");
  if (!rc && spoil) { // tests: the transforms get a table whose first row is negated in every orbit -- no longer the basis the blocks were built in
    std::vector<double> bad = tabp;
    for (int o = 0; o < B.norb; o++)
      for (int j = 0; j < B.osize[o]; j++) bad[(size_t)toffp[o] + j] = -bad[(size_t)toffp[o] + j];
    rc = pmh_memcpy_h2d(ctx, a->d_tab, bad.data(), sizeof(double) * bad.size());
    tabp.swap(bad);
  }
  if (!rc && a->narrow) { // k_fxa_narrow's two copies (fxn_tab_off: the order its waves load in), of whichever table the wide kernels would read
    std::vector<double> tabN(tabp.size()), tabNT(tabp.size());
    for (int o = 0; o < B.norb; o++)
      for (int t = 0; t < 48; t++)
        for (int j = 0; j < 48; j++) {
          const double v = tabp[(size_t)toffp[o] + t * 48 + j];
          tabN[(size_t)toffp[o] + fxn_tab_off(t, j)] = v, tabNT[(size_t)toffp[o] + fxn_tab_off(j, t)] = v;
        }
    rc = fxa_upload(ctx, tabN, &a->d_tabN);
    if (!rc) rc = fxa_upload(ctx, tabNT, &a->d_tabNT);
  }
  return rc;
}

// After the assembly: every eligible class gets its symmetry-adapted form, then ONE random multivector goes through both that form and the GEMM -- a blunder detector:
// a wrong basis is wrong by O(1), rounding is 1e-15, the bound of 1e-10 sits five orders from either.  A class that misses it stays on the GEMM (counter
// orbit_adapted_fallbacks).  One rank only (the several-rank k-range split keeps the GEMM); any PMH_FXO_* switch steers the GEMM, so it selects the GEMM.
static int fxa_setup(fx_shared *S)
{
  pmh_ctx ctx = S->ctx;
  for (fxs_class &C : S->C) fxa_free(ctx, C);
  if (!pmh_knobs().orbit_adapted || S->stripe_size > 1 || ctx->size > 1) return PMH_SUCCESS;
  for (char **e = environ; e && *e; e++)
    if (!strncmp(*e, "PMH_FXO_", 8)) return PMH_SUCCESS;
  const bool spoil = pmh_knobs().orbit_adapted_spoil != 0;
  pmh_knobs().orbit_adapted_spoil = 0;
  bool any = false;
  for (fxs_class &C : S->C) {
    if (!C.nc) continue;
    // (records of fewer than 8 slots -- classes of fewer than 8 blocks -- keep the GEMM)
    if (C.S != FXS_S || C.nsym != OAB_NOP || C.h_ops.size() != 6 * (size_t)OAB_NOP || C.m0 != 0 || C.m1 != C.M_all || C.tmask.empty()) {
      if (getenv("PMH_ORBIT_ADAPTED_VERBOSE")) fprintf(stderr, "orbit_adapted: not eligible (slots %d, operations %d, box operations known %d): the class keeps the GEMM\n", C.S, C.nsym, (int)(C.h_ops.size() / 6));
      continue;
    }
    const int rc = fxa_build_class(S, C, spoil);
    if (rc) {
      fxa_free(ctx, C);
      return rc;
    }
    any = any || C.oa;
  }
  if (!any) return PMH_SUCCESS;
  std::vector<double> x((size_t)S->nX, 0.0), y0((size_t)S->nX), y1((size_t)S->nX);
  unsigned long long  seed = 0x9E3779B97F4A7C15ULL;
  for (fxs_class &C : S->C) {
    if (!C.oa) continue;
    for (int g = 0; g < C.ngroups; g++)
      for (int p = 0; p < C.nc; p++)
        for (int sl = 0; sl < FXS_S; sl++)
          if (C.tmask[((size_t)g * C.nc + p) * FXS_S + sl]) {
            seed = seed * 6364136223846793005ULL + 1442695040888963407ULL;
            x[(size_t)(C.xoff + (long long)g * C.ld * FXS_S + (long long)p * FXS_S + sl)] = (double)(seed >> 11) / 4503599627370496.0 - 1.0;
          }
  }
  PMH_CHK(pmh_memcpy_h2d(ctx, S->X, x.data(), sizeof(double) * x.size()));
  for (const fxs_class &C : S->C) {
    const long long n = (long long)C.ngroups * C.ld * C.S;
    if (!n) continue;
    hipLaunchKernelGGL(k_fxo_signed_copy, dim3((unsigned)std::min<long long>(4096, (n + PMH_BLOCK - 1) / PMH_BLOCK)), dim3(PMH_BLOCK), 0, ctx->stream, n, C.S, (const double *)(S->X + C.xoff), S->X2 + 2 * C.xoff);
  }
  PMH_CHK(fxo_gemm(S));
  PMH_CHK(pmh_memcpy_d2h(ctx, y0.data(), S->Y, sizeof(double) * y0.size()));
  PMH_CHK(pmh_memset(ctx, S->Y, 0, sizeof(double) * (size_t)S->nX));
  PMH_CHK(fxa_launch(S));
  PMH_CHK(pmh_memcpy_d2h(ctx, y1.data(), S->Y, sizeof(double) * y1.size()));
  for (fxs_class &C : S->C) {
    if (!C.oa) continue;
    double dd = 0.0, nn = 0.0;
    for (int g = 0; g < C.ngroups; g++) // where some block reads Y (both forms leave every other entry zero)
      for (long long k = 0; k < (long long)C.nc * FXS_S; k++)
        if (C.tmask[(size_t)g * C.nc * FXS_S + (size_t)k]) {
          const size_t i = (size_t)(C.xoff + (long long)g * C.ld * FXS_S + k);
          dd += (y1[i] - y0[i]) * (y1[i] - y0[i]), nn += y0[i] * y0[i];
        }
    if (getenv("PMH_ORBIT_ADAPTED_VERBOSE")) fprintf(stderr, "orbit_adapted: self-check against the GEMM: normwise relative difference %.3e (n_c = %d, %d groups)\n", std::sqrt(dd / nn), C.nc, C.ngroups);
    if (!(dd <= 1e-20 * nn)) fxa_free(ctx, C), pmh_knobs().orbit_adapted_fallbacks++;
    else pmh_knobs().orbit_adapted_classes++;
  }
  // the multivectors as the operator expects them: zero wherever its own gluing does not write
  PMH_CHK(pmh_memset(ctx, S->X, 0, sizeof(double) * (size_t)S->nX));
  PMH_CHK(pmh_memset(ctx, S->X2, 0, sizeof(double) * 2 * (size_t)S->nX));
  PMH_CHK(pmh_memset(ctx, S->Y, 0, sizeof(double) * (size_t)S->nX));
  return pmh_sync(ctx);
}

// ---- the set-up: what each storage form hands the loop of fx_assemble.h (its columns, its row writer, its self-check), chosen once per call -------------------------
static inline int     fxs_row_grid(int n) { return std::max(1, std::min(64, (n + PMH_BLOCK - 1) / PMH_BLOCK)); }
static inline double *fxs_super_band(fx_shared *S, const fxs_class &C, int row) // the first tile of the row's super band (symmetric tiles)
{
  const long long sb = row / FXM_RS;
  return S->Wbase + C.woff + (long long)FXM_RS * FXM_RS * (sb * (sb + 1) / 2);
}
// orbit storage: a row of W_c (u[rel[i]], i < n_c) into row `row` of the pre-tiled A
static void fxo_store_row(fx_shared *S, const fxs_class &C, int row, const int *d_rel, const double *u)
{
  hipLaunchKernelGGL(k_fxo_store_row, dim3(fxs_row_grid(C.nc)), dim3(PMH_BLOCK), 0, S->ctx->stream, row, C.tm, C.nc, C.nkc, d_rel, (const int *)C.d_kinv, u, S->Afund + C.aoff);
}

// PMH_FX_CLASS: the rows of this rank's stripe, each stored in full
static void fxs_plan_full(fx_shared *S, fx_asm_plan &P)
{
  for (int c = 0; c < S->ncls; c++) {
    const fxs_class &C = S->C[c];
    for (int p = C.r0; p < std::min(C.r1, C.nc); p++) P.todo[c].push_back({C.urel[p], p});
  }
  P.write = [S](int c, int p, const double *u) { // row p of W_c = column p (K^+ symmetric)
    const fxs_class &C = S->C[c];
    fx_extract_row(S->ctx, C.nc, C.d_urel, u, S->Wbase + C.woff + (long long)p * C.ld);
  };
}

// PMH_FX_CLASS_SYM: the rows of this rank's super bands.  A class with symmetries solves one row per orbit that has a row there and fills the orbit's owned rows from it;
// symmetry-filled rows are the self-check's candidates.
static void fxs_plan_tiles(fx_shared *S, fx_asm_plan &P)
{
  std::vector<std::map<int, std::vector<std::pair<int, int>>>> members(S->ncls); // per class with symmetries: representative row -> (owned row of its orbit, the operation that reaches it)
  for (int c = 0; c < S->ncls; c++) {
    const fxs_class &C = S->C[c];
    if (C.nsym <= 1) {
      for (int p = 0; p < C.nc; p++)
        if (C.own[p / FXM_RS]) P.todo[c].push_back({C.urel[p], p});
      continue;
    }
    std::vector<int> rep_of((size_t)C.nc, -1), op_of((size_t)C.nc, 0);
    for (int p = 0; p < C.nc; p++) {
      if (rep_of[p] >= 0) continue;
      for (int g = 0; g < C.nsym; g++) {
        const int r = C.h_posmap[(size_t)g * C.nc + p];
        if (rep_of[r] < 0) rep_of[r] = p, op_of[r] = g;
      }
    }
    for (int r = 0; r < C.nc; r++)
      if (C.own[r / FXM_RS]) {
        members[c][rep_of[r]].push_back({r, op_of[r]});
        if (op_of[r] != 0) P.check[c].push_back({C.urel[r], r});
      }
    for (const auto &m : members[c]) P.todo[c].push_back({C.urel[m.first], m.first}); // (ascending)
  }
  P.write = [S, members = std::move(members)](int c, int p, const double *u) {
    const fxs_class &C = S->C[c];
    if (members[c].empty()) {
      hipLaunchKernelGGL(k_fxs_extract_sym, dim3(fxs_row_grid(p + 1)), dim3(PMH_BLOCK), 0, S->ctx->stream, p, (const int *)C.d_urel, u, fxs_super_band(S, C, p));
      return;
    }
    for (const auto &rg : members[c].at(p)) {
      const int r = rg.first, g = rg.second;
      hipLaunchKernelGGL(k_fxs_extract_symg, dim3(fxs_row_grid(C.nc)), dim3(PMH_BLOCK), 0, S->ctx->stream, r, C.nc, (double)C.h_sign[(size_t)g * C.nc + p], (const int *)C.d_urel, u,
                         (const int *)(C.d_posmap + (size_t)g * C.nc), (const signed char *)(C.d_sign + (size_t)g * C.nc), fxs_super_band(S, C, r));
    }
  };
  P.check_row = [S](int c, int r, const double *u, double *d_out) {
    const fxs_class &C = S->C[c];
    hipLaunchKernelGGL(k_fxs_check_row, dim3(fxs_row_grid(r + 1)), dim3(PMH_BLOCK), 0, S->ctx->stream, r, (const int *)C.d_urel, u, (const double *)fxs_super_band(S, C, r), d_out);
    return fxs_row_grid(r + 1);
  };
}

// PMH_FX_CLASS_ORBIT (after fxo_prepare): the owned representatives' rows; self-check candidates: rows of their orbits reached by a non-trivial operation
static void fxs_plan_orbit(fx_shared *S, fx_asm_plan &P)
{
  for (int c = 0; c < S->ncls; c++) {
    const fxs_class &C = S->C[c];
    if (!C.nc) continue;
    for (int pl = 0; pl < C.m1 - C.m0; pl++) P.todo[c].push_back({C.urel[C.reps[C.m0 + pl]], pl});
    for (int r = 0; r < C.nc; r++)
      if (C.op_of[r] != 0) {
        const int k = (int)(std::lower_bound(C.reps.begin(), C.reps.end(), C.rep_of[r]) - C.reps.begin());
        if (k >= C.m0 && k < C.m1) P.check[c].push_back({C.urel[r], r});
      }
  }
  P.write     = [S](int c, int pl, const double *u) { fxo_store_row(S, S->C[c], S->C[c].reprow[pl], S->C[c].d_urel, u); };
  P.check_row = [S](int c, int r, const double *u, double *d_out) {
    const fxs_class &C = S->C[c];
    const int        g = C.op_of[r], p = C.rep_of[r], pl = (int)(std::lower_bound(C.reps.begin(), C.reps.end(), p) - C.reps.begin()) - C.m0;
    hipLaunchKernelGGL(k_fxo_check_row, dim3(fxs_row_grid(C.nc)), dim3(PMH_BLOCK), 0, S->ctx->stream, C.reprow[pl], C.tm, C.nc, C.nkc, (double)C.h_sign[(size_t)g * C.nc + p], (const int *)C.d_urel,
                       (const int *)C.d_kinv, u, (const int *)(C.d_posmap + (size_t)g * C.nc), (const signed char *)(C.d_sign + (size_t)g * C.nc), (const double *)(S->Afund + C.aoff), d_out);
    return fxs_row_grid(C.nc);
  };
}

int fxs_assemble(fx_shared *S, pmh_matinv solver, int nslots, const int *slot_class, double rtol, int max_it, long long *n_solves, fx_batch_window *w)
{
  PMH_ARG(S && solver && nslots >= 1 && (solver->nblocks == nslots || solver->nblocks * PMH_MV_R == nslots) && slot_class);
  if (S->sym == 2) PMH_CHK(fxo_prepare(S));
  fx_asm_plan P(S->ncls);
  for (int c = 0; c < S->ncls; c++)
    if (S->C[c].nc) P.nloc[c] = S->C[c].nloc;
  if (S->sym == 2) fxs_plan_orbit(S, P);
  else if (S->sym) fxs_plan_tiles(S, P);
  else fxs_plan_full(S, P);
  PMH_CHK(fx_assemble_run(S->ctx, P, solver, nslots, slot_class, rtol, max_it, n_solves, w));
  if (S->sym == 2 && (!w || w->complete)) return fxa_setup(S); // every representative's row is there: the symmetry-adapted form
  return PMH_SUCCESS;
}

static int fxs_gemm(fx_shared *S)
{
  if (S->sym == 2 && !S->fxo_ready) return pmh_set_error(PMH_ERR_STATE, "PMH_FX_CLASS_ORBIT: apply before the assembly");
  if (!S->nwg) return PMH_SUCCESS;
  hipStream_t st    = S->ctx->stream;
  const bool  timed = S->ev_on && (size_t)(2 * S->ev_used + 2) <= S->ev.size();
  if (timed) PMH_HIP(hipEventRecord(S->ev[2 * S->ev_used], st));
  const long long stride = std::max(16LL, S->nX);
  if (S->sym == 2) {
    S->ev_mid_pending = timed ? S->ev_used : -1;
    if (fxa_active(S)) PMH_CHK(fxa_launch(S));
    else PMH_CHK(fxo_gemm(S));
    S->ev_mid_pending = -1;
  } else if (S->sym) {
    hipLaunchKernelGGL(k_fxs_symm8, dim3(S->nwg), dim3(FXM_THREADS), 0, st, (const int *)S->d_wg, (const int *)S->d_items, (const long long *)S->d_wgl, (const int *)S->d_ld, (const long long *)S->d_xoff,
                       (const double *)S->Wbase, (const double *)S->X, S->part, stride, S->pt);
    for (auto &C : S->C)
      if (C.ld) // (a class B does not touch has no entry of Y: a grid of 0 workgroups is not a launch)
        hipLaunchKernelGGL(k_fxs_symfin, dim3((unsigned)(((long long)C.ld * FXS_S / 2 * 8 + PMH_BLOCK - 1) / PMH_BLOCK), C.ngroups), dim3(PMH_BLOCK), 0, st, C.ld, C.nmb, C.nown, (const int *)C.d_nseg, (const int *)C.d_ownfirst,
                         (const long long *)C.d_ptoff, C.xoff, stride, (const double *)S->part, (const double *)S->pt, S->Y);
  } else {
  hipLaunchKernelGGL(k_fxs_gemm8, dim3(S->nwg), dim3(PMH_BLOCK), 0, st, (const int *)S->d_wg, (const int *)S->d_ld, (const long long *)S->d_woff, (const long long *)S->d_xoff, (const double *)S->Wbase,
                     (const double *)S->X, S->part, stride);
  hipLaunchKernelGGL(k_fxs_fin, dim3((unsigned)((S->nX / 2 + PMH_BLOCK - 1) / PMH_BLOCK)), dim3(PMH_BLOCK), 0, st, S->nX, S->nseg, stride, (const double *)S->part, S->Y);
  }
  if (timed) {
    PMH_HIP(hipEventRecord(S->ev[2 * S->ev_used + 1], st));
    S->ev_used++;
  }
  PMH_HIP(hipGetLastError());
  return PMH_SUCCESS;
}

int fxs_apply(fx_shared *S, const double *lambda, double *y)
{
  if (S->sym == 2) PMH_CHK(pmh_gluing_mult(S->Bc2, lambda, S->X2));
  else PMH_CHK(pmh_gluing_mult(S->Bc, lambda, S->X));
  PMH_CHK(fxs_gemm(S));
  return pmh_gluing_mult_transpose(S->Bc, S->Y, y); // ends with the all-reduce on several GPUs
}

int fxs_stages(fx_shared *S, pmh_csr *gather, double **mid_in, pmh_csr *scatter, const double **mid_out)
{
  if (S->sym == 2) *gather = S->Bc2->Bt, *mid_in = S->X2;
  else *gather = S->Bc->Bt, *mid_in = S->X;
  *scatter = S->Bc->B, *mid_out = S->Y;
  return PMH_SUCCESS;
}
int fxs_mid(fx_shared *S) { return fxs_gemm(S); }

// the dense kernel alone (tests, tuning): Y = blockdiag(W_c) X on the multivectors as they stand
int fxs_dense(fx_shared *S)
{
  if (S->sym == 2 && S->nX > 0) {
    for (const fxs_class &C : S->C) { // class by class: the records of a class have C.S slots
      const long long n = (long long)C.ngroups * C.ld * C.S;
      if (!n) continue;
      hipLaunchKernelGGL(k_fxo_signed_copy, dim3((unsigned)std::min<long long>(4096, (n + PMH_BLOCK - 1) / PMH_BLOCK)), dim3(PMH_BLOCK), 0, S->ctx->stream, n, C.S, (const double *)(S->X + C.xoff), S->X2 + 2 * C.xoff);
    }
    PMH_HIP(hipGetLastError());
  }
  return fxs_gemm(S);
}
long long fxs_multivector_length(fx_shared *S) { return S->nX; }
double   *fxs_X(fx_shared *S) { return S->X; }
double   *fxs_Y(fx_shared *S) { return S->Y; }

int fxs_fill_pattern(fx_shared *S, int byte)
{
  if (S->sym == 2) {
    PMH_CHK(fxo_prepare(S));
    PMH_HIP(hipMemsetAsync(S->Afund, byte, sizeof(double) * (size_t)S->afund_tot, S->ctx->stream));
    return pmh_sync(S->ctx);
  }
  PMH_HIP(hipMemsetAsync(S->Wbase, byte, sizeof(double) * (size_t)S->wtot, S->ctx->stream));
  return pmh_sync(S->ctx);
}

// W_b = W_c[pos_b, pos_b] on the host (tests); gamma: the block's touched dofs (rank-local primal indices, ascending)
int fxs_get_block(fx_shared *S, int b, int n, const int *gamma, double *out_host)
{
  const fxs_class    &C = S->C[S->cls[b]];
  if (S->sym == 2) {
    // orbit storage (tests: small classes, all representatives on this rank): row r = g p rebuilt from its representative's row
    if (!S->fxo_ready || C.m0 != 0 || C.m1 != C.M_all) return pmh_set_error(PMH_ERR_STATE, "pmh_fexplicit_get_block: the orbit storage holds only this rank's representatives");
    std::vector<double> T((size_t)C.Mp * C.ldk), row((size_t)C.nc);
    PMH_HIP(hipMemcpy(T.data(), S->Afund + C.aoff, sizeof(double) * T.size(), hipMemcpyDeviceToHost));
    for (int i = 0; i < n; i++) {
      const int r = C.pos[gamma[i] - S->K->rowstart[b]], p = C.rep_of[r], g = C.op_of[r], pl = (int)(std::lower_bound(C.reps.begin(), C.reps.end(), p) - C.reps.begin());
      const double  sp = (double)C.h_sign[(size_t)g * C.nc + p];
      const int     pr = C.reprow[pl]; // the representative's row of A
      const double *ab = T.data() + (size_t)(pr / C.tm) * C.nkc * (FXO_TK * C.tm) + pr % C.tm;
      for (int cc = 0; cc < C.nc; cc++) {
        const int k = C.kinv[cc];
        row[C.h_posmap[(size_t)g * C.nc + cc]] = sp * (double)C.h_sign[(size_t)g * C.nc + cc] * ab[(size_t)(k / FXO_TK) * (FXO_TK * C.tm) + (k % FXO_TK) * C.tm];
      }
      for (int k = 0; k < n; k++) out_host[(size_t)i * n + k] = row[C.pos[gamma[k] - S->K->rowstart[b]]];
    }
    return PMH_SUCCESS;
  }
  if (S->sym) {
    // the class's tiles on the host (tests: small classes), W[p][c] from the stored lower triangle
    const long long     len = (long long)FXM_RS * FXM_RS * ((long long)C.nsb * (C.nsb + 1) / 2);
    std::vector<double> T((size_t)len);
    PMH_HIP(hipMemcpy(T.data(), S->Wbase + C.woff, sizeof(double) * (size_t)len, hipMemcpyDeviceToHost));
    auto at = [&](int p, int c) {
      const int hi = std::max(p, c), lo = std::min(p, c), sb = hi / FXM_RS, Il = (hi % FXM_RS) / 16, r = hi & 15, q = r >> 2, l = 16 * (r & 3) + (lo & 15);
      const double v = T[(size_t)((long long)FXM_RS * FXM_RS * ((long long)sb * (sb + 1) / 2) + ((long long)(lo >> 4) * FXM_RT + Il) * 256 + (q >> 1) * 128 + 2 * l + (q & 1))];
      return hi == lo ? 2.0 * v : v;
    };
    for (int i = 0; i < n; i++)
      for (int k = 0; k < n; k++) out_host[(size_t)i * n + k] = at(C.pos[gamma[i] - S->K->rowstart[b]], C.pos[gamma[k] - S->K->rowstart[b]]);
    return PMH_SUCCESS;
  }
  std::vector<double> row((size_t)std::max(1, C.ld));
  for (int i = 0; i < n; i++) {
    const int p = C.pos[gamma[i] - S->K->rowstart[b]];
    PMH_HIP(hipMemcpy(row.data(), S->Wbase + C.woff + (long long)p * C.ld, sizeof(double) * (size_t)C.ld, hipMemcpyDeviceToHost));
    for (int k = 0; k < n; k++) out_host[(size_t)i * n + k] = row[C.pos[gamma[k] - S->K->rowstart[b]]];
  }
  return PMH_SUCCESS;
}

// ---- orbit storage: test entries (pmh_fexplicit_test_load_class / pmh_fexplicit_orbit_plan_info) ---------------------------------------------------------------
// The representatives' rows of class c from a HOST matrix W (n_c x n_c, row-major, in the numbering of fxs_class_union) instead of K^+ solves: the plan as the
// assembly makes it (fxo_prepare), row reps[pl] stored through k_fxo_store_row into row reprow[pl] of the pre-tiled A.  No solver, no symmetry-adapted form.
// *all_loaded: every class with touched dofs has its rows.
int fxs_test_load_class(fx_shared *S, int c, const double *W, int *all_loaded)
{
  PMH_ARG(S && W && all_loaded && c >= 0 && c < S->ncls);
  if (S->sym != 2) return pmh_set_error(PMH_ERR_ARG, "pmh_fexplicit_test_load_class: needs the PMH_FX_CLASS_ORBIT storage");
  pmh_ctx    ctx = S->ctx;
  if (!S->fxo_ready) // a new plan: its A starts from zero
    for (fxs_class &D : S->C) D.test_loaded = 0;
  PMH_CHK(fxo_prepare(S)); // PMH_ERR_STATE: a class with touched dofs has no symmetries yet
  fxs_class &C = S->C[c];
  const int  M = C.m1 - C.m0;
  if (C.nc) {
    std::vector<double> rows((size_t)M * C.nc);
    std::vector<int>    ident((size_t)C.nc);
    for (int pl = 0; pl < M; pl++) memcpy(&rows[(size_t)pl * C.nc], W + (size_t)C.reps[C.m0 + pl] * C.nc, sizeof(double) * (size_t)C.nc);
    for (int i = 0; i < C.nc; i++) ident[i] = i;
    double *d_rows = nullptr;
    int    *d_ident = nullptr;
    PMH_CHK(pmh_malloc(ctx, sizeof(double) * rows.size(), (void **)&d_rows));
    int rc = pmh_malloc(ctx, sizeof(int) * ident.size(), (void **)&d_ident);
    if (!rc) rc = pmh_memcpy_h2d(ctx, d_rows, rows.data(), sizeof(double) * rows.size());
    if (!rc) rc = pmh_memcpy_h2d(ctx, d_ident, ident.data(), sizeof(int) * ident.size());
    for (int pl = 0; pl < M && !rc; pl++)
      fxo_store_row(S, C, C.reprow[pl], d_ident, d_rows + (size_t)pl * C.nc);
    if (!rc && hipGetLastError() != hipSuccess) rc = pmh_set_error(PMH_ERR_HIP, "pmh_fexplicit_test_load_class: launch failed");
    if (!rc) rc = pmh_sync(ctx);
    if (d_rows) pmh_free(ctx, d_rows);
    if (d_ident) pmh_free(ctx, d_ident);
    if (rc) return rc;
  }
  C.test_loaded = 1;
  *all_loaded = 1;
  for (const fxs_class &D : S->C)
    if (D.nc && !D.test_loaded) *all_loaded = 0;
  return PMH_SUCCESS;
}

// ---- PMH_FX_CLASS / PMH_FX_CLASS_SYM: test entries (pmh_fexplicit_test_load_rows / _test_info / _test_read_storage) -------------------------------------------
// Rows [row0, row0 + nrows) of W_c from a HOST matrix (rows of n_c doubles in the numbering of fxs_class_union), stored by the write function of the plan the assembly
// makes (fxs_plan_full / fxs_plan_tiles): each row goes to the device in block-relative dof numbering, so the store kernels gather through d_urel as they do from a
// K^+ solution.  Rows outside the plan (another rank's stripe; with symmetries: rows that are no representative) are skipped, as the assembly never solves for them.
int fxs_test_load_rows(fx_shared *S, int c, int row0, int nrows, const double *rows_host, int *all_loaded)
{
  PMH_ARG(S && rows_host && all_loaded && c >= 0 && c < S->ncls && row0 >= 0 && nrows >= 0);
  if (S->sym == 2) return pmh_set_error(PMH_ERR_ARG, "pmh_fexplicit_test_load_rows: the orbit storage loads through pmh_fexplicit_test_load_class");
  pmh_ctx    ctx = S->ctx;
  fxs_class &C   = S->C[c];
  PMH_ARG(row0 + nrows <= C.nc);
  C.test_rows.resize((size_t)C.nc, 0);
  if (nrows) {
    fx_asm_plan P(S->ncls);
    if (S->sym) fxs_plan_tiles(S, P);
    else fxs_plan_full(S, P);
    std::vector<char> todo((size_t)C.nc, 0);
    for (const fx_asm_row &t : P.todo[c]) todo[t.id] = 1;
    std::vector<double> U((size_t)nrows * C.nloc, 0.0);
    for (int k = 0; k < nrows; k++)
      for (int i = 0; i < C.nc; i++) U[(size_t)k * C.nloc + C.urel[i]] = rows_host[(size_t)k * C.nc + i];
    double *dU = nullptr;
    PMH_CHK(pmh_malloc(ctx, sizeof(double) * U.size(), (void **)&dU));
    int rc = pmh_memcpy_h2d(ctx, dU, U.data(), sizeof(double) * U.size());
    for (int k = 0; k < nrows && !rc; k++)
      if (todo[row0 + k]) P.write(c, row0 + k, dU + (size_t)k * C.nloc);
    if (!rc && hipGetLastError() != hipSuccess) rc = pmh_set_error(PMH_ERR_HIP, "pmh_fexplicit_test_load_rows: launch failed");
    if (!rc) rc = pmh_sync(ctx);
    pmh_free(ctx, dU);
    if (rc) return rc;
    for (int k = 0; k < nrows; k++) C.test_rows[row0 + k] = 1;
  }
  *all_loaded = 1;
  for (const fxs_class &D : S->C)
    if (D.nc && ((int)D.test_rows.size() != D.nc || std::find(D.test_rows.begin(), D.test_rows.end(), 0) != D.test_rows.end())) *all_loaded = 0;
  return PMH_SUCCESS;
}

// what the launch tables of the two streaming class storages hold for class c (the layout of info: include/permon_hip.h); reads state only
int fxs_test_info(fx_shared *S, int c, long long info[80])
{
  PMH_ARG(S && info && c >= 0 && c < S->ncls);
  const fxs_class &C = S->C[c];
  info[1] = C.nc, info[2] = C.ld, info[10] = C.xoff, info[11] = C.woff, info[12] = C.ngroups;
  if (!S->sym) { // bands: the row groups of 32 the stripes are dealt in
    info[3] = C.ld / 32;
    for (int k = C.r0 / 32; k < C.r1 / 32; k++) {
      info[4]++;
      if (k < 64) info[16 + k] = 1;
    }
    info[5] = S->nseg, info[6] = C.r0, info[7] = C.r1, info[8] = S->nwg;
    return PMH_SUCCESS;
  }
  info[3] = C.nmb, info[9] = C.nsb;
  for (int m = 0; m < C.nmb; m++)
    if (C.own[FXM_MB * m]) {
      info[4]++;
      if (m < 64) info[16 + m] = 1;
    }
  info[5] = S->nwg, info[6] = S->nitems, info[7] = C.nseg_max;
  return PMH_SUCCESS;
}

int fxs_test_read_storage(fx_shared *S, long long offset, long long count, double *out_host)
{
  PMH_ARG(S && out_host && S->sym != 2 && offset >= 0 && count >= 0 && offset + count <= S->wtot);
  return count ? pmh_memcpy_d2h(S->ctx, out_host, S->Wbase + offset, sizeof(double) * (size_t)count) : PMH_SUCCESS;
}

// what fxo_prepare decided for class c and what fxo_gemm launches for it (the layout of info: include/permon_hip.h)
int fxs_orbit_plan_info(fx_shared *S, int c, long long info[24])
{
  PMH_ARG(S && info && c >= 0 && c < S->ncls);
  if (S->sym != 2) return pmh_set_error(PMH_ERR_ARG, "pmh_fexplicit_orbit_plan_info: needs the PMH_FX_CLASS_ORBIT storage");
  if (!S->fxo_ready) return pmh_set_error(PMH_ERR_STATE, "pmh_fexplicit_orbit_plan_info: no plan yet (after the assembly or pmh_fexplicit_test_load_class)");
  const fxs_class &C    = S->C[c];
  const int        kind = fxo_launch_kind(S, C);
  if (C.nc && !(kind == 2 ? fxo_instance(S->merged_tm, S->merged_tn, S->merged_tnw, true) : fxo_instance(C.tm, C.tn, C.tnw, kind == 1)))
    return pmh_set_error(PMH_ERR_STATE, "PMH_FX_CLASS_ORBIT: row tile %d has no 16x16x4 kernel", C.tm);
  const long long v[24] = {C.nc, C.ld, C.S, C.ngroups, C.xoff, C.nsym, C.nsymp, C.M_all, C.tm, C.Mp, C.nc ? C.Mp / C.tm : 0, C.tn, C.tnw, C.nseg, C.nkc, C.plan_units, C.plan_units_work, C.plan_smax,
                           C.wg_count, C.plan_wg2, kind, S->d_fin_args ? 1 : 0, C.m0, C.m1};
  memcpy(info, v, sizeof(v));
  return PMH_SUCCESS;
}

// what k_fxa_prod runs for class c in the symmetry-adapted form (the layout of info: include/permon_hip.h); called by nothing inside the solvers
int fxs_orbit_adapted_info(fx_shared *S, int c, long long info[200])
{
  PMH_ARG(S && info && c >= 0 && c < S->ncls);
  if (!fxs_orbit_adapted(S, c)) return pmh_set_error(PMH_ERR_STATE, "pmh_fexplicit_orbit_adapted_info: class %d does not apply W_c in the symmetry-adapted basis", c);
  const fxa_class *a = S->C[c].oa;
  memset(info, 0, sizeof(long long) * 200);
  for (int i = 0; i < OAB_NIRREP; i++) {
    const fxa_irrep &I = a->ir[i];
    long long       *v = info + 20 * i;
    v[0] = I.d, v[1] = I.m, v[2] = I.nks, v[3] = I.nob, v[4] = I.nbt, v[19] = a->narrow;
    for (int nbw = 1; nbw <= 4; nbw++) v[4 + nbw] = a->items_of_width[i][nbw - 1];
    for (int wide = 0; wide < 2; wide++) {
      const int U = fxa_trip_steps(wide ? 4 : 1);
      v[17 + wide] = U;
      for (int w = 0; w < FXA_WAVES; w++) v[9 + 4 * wide + w] = (fxa_wave_k0(I.nks, U, w + 1) - fxa_wave_k0(I.nks, U, w)) / U;
    }
  }
  return PMH_SUCCESS;
}

// tests: ONE transform of class c, launched as fxa_launch launches it; X^ / Y^ cross the interface as (basis function, column).  Called by nothing inside the solvers
int fxs_orbit_adapted_transform(fx_shared *S, int c, int inverse, const double *in, double *out)
{
  PMH_ARG(S && in && out && c >= 0 && c < S->ncls);
  if (!fxs_orbit_adapted(S, c)) return pmh_set_error(PMH_ERR_STATE, "pmh_fexplicit_orbit_adapted_transform: class %d does not apply W_c in the symmetry-adapted basis", c);
  pmh_ctx          ctx = S->ctx;
  const fxs_class &C   = S->C[c];
  const fxa_class *a   = C.oa;
  const long long  n   = (long long)C.nc * a->NC, ncopy = (long long)C.ngroups * C.ld * C.S;
  const unsigned   nbx = (unsigned)((n + PMH_BLOCK - 1) / PMH_BLOCK);
  if (inverse) {
    PMH_CHK(pmh_memset(ctx, S->Y, 0, sizeof(double) * (size_t)S->nX));
    hipLaunchKernelGGL(k_fxa_logical<true>, dim3(nbx), dim3(PMH_BLOCK), 0, ctx->stream, (const fxa_irrep *)a->d_ir, (const int *)a->d_rowinfo, C.nc, a->NC, in, a->Yh);
    fxa_launch_transform(S, C, true);
    PMH_HIP(hipGetLastError());
    return pmh_memcpy_d2d(ctx, out, S->Y, sizeof(double) * (size_t)S->nX);
  }
  PMH_CHK(pmh_memcpy_d2d(ctx, S->X, in, sizeof(double) * (size_t)S->nX));
  hipLaunchKernelGGL(k_fxo_signed_copy, dim3((unsigned)std::min<long long>(4096, (ncopy + PMH_BLOCK - 1) / PMH_BLOCK)), dim3(PMH_BLOCK), 0, ctx->stream, ncopy, C.S, (const double *)(S->X + C.xoff), S->X2 + 2 * C.xoff);
  fxa_launch_transform(S, C, false);
  hipLaunchKernelGGL(k_fxa_logical<false>, dim3(nbx), dim3(PMH_BLOCK), 0, ctx->stream, (const fxa_irrep *)a->d_ir, (const int *)a->d_rowinfo, C.nc, a->NC, (const double *)a->Xh, out);
  PMH_HIP(hipGetLastError());
  return pmh_sync(ctx);
}

int fxs_timing_enable(fx_shared *S, int max_launches)
{
  while ((int)S->ev.size() < 2 * max_launches) {
    hipEvent_t e;
    PMH_HIP(hipEventCreate(&e));
    S->ev.push_back(e);
  }
  while ((int)S->ev_mid.size() < max_launches) {
    hipEvent_t e;
    PMH_HIP(hipEventCreate(&e));
    S->ev_mid.push_back(e);
  }
  S->ev_on = max_launches > 0, S->ev_used = 0;
  return PMH_SUCCESS;
}

int fxs_timing_get(fx_shared *S, int *launches, double *total_ms, double *first_kernel_ms)
{
  PMH_CHK(pmh_sync(S->ctx));
  double tot = 0.0, first = 0.0;
  for (int i = 0; i < S->ev_used; i++) {
    float ms = 0.f;
    PMH_HIP(hipEventElapsedTime(&ms, S->ev[2 * i], S->ev[2 * i + 1]));
    tot += ms;
    if (S->sym == 2) {
      PMH_HIP(hipEventElapsedTime(&ms, S->ev[2 * i], S->ev_mid[i]));
      first += ms;
    }
  }
  *launches = S->ev_used, *total_ms = tot;
  if (first_kernel_ms) *first_kernel_ms = S->sym == 2 ? first : tot; // orbit storage: the GEMM kernel alone (the rest is k_fxo_fin)
  return PMH_SUCCESS;
}
