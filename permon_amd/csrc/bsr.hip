// 3x3-block sparse matrix-vector product for the elasticity blocks K_i (PETSc's SeqBAIJ role, bs = 3) in a
// device-private layout.  A CSR row of K_i costs 12 bytes per non-zero (fp64 value + int32 column); with one column index
// per 3x3 block it is 8.44 (fp64 values), 4.44 (fp32) or 2.44 (fp16 values, fp32 arithmetic) -- the reduced precisions are
// used only inside the multigrid preconditioner.  The kernel is HBM bound, so the byte count is the run time.
//
// Layout: block rows are grouped into tiles of at most 1024 blocks (512 on the coarse multigrid levels; whole block rows per
// tile, block count padded to a multiple of the load width W = bsr_w<entry type> with zero blocks); inside a tile the nine
// entries of the blocks are stored as nine planes of length nbp (structure of arrays), so that a thread reads entry k of its
// W adjacent blocks with one W-wide load at plane k: every load of the value stream is lane-contiguous.  One workgroup per
// tile: each thread multiplies its blocks with the three x entries of the block column, writes the three partial products to
// LDS, then four lanes per scalar row add the row's partials in a fixed order (deterministic, no atomics).
#include "pmh_internal.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <memory>
#include <thread>

// adjacent blocks per load: 16-byte loads of fp64 / fp32 entries, 8-byte loads of fp16 entries (profiles/r01_bsr3_tune.txt)
template <typename TM> constexpr int bsr_w = sizeof(TM) == 8 ? 2 : 4;

// Epilogues.  Besides y = A x (+/- y1) the kernel can finish a Chebyshev/Jacobi smoothing step of the V-cycle on the row it
// has just summed, which removes the separate vector kernels (and their launches) from the cycle.  All fused variants write
// to vectors that no workgroup gathers from during the same launch.
//   PRE   (x = d0 gathered):  y = c0 d0 + c2 dinv (b - A d0)                      second step of the zero-guess pre-smoother
//   POST1 (x gathered):       r = dinv (b - A x); d = c0 r; y = x + d             first step of the post-smoother
//   POST2 (x = d gathered):   y += c1 d + c2 (r - dinv A d); optional fp64 copy   second step of the post-smoother
// TM: storage type of the matrix entries, T: arithmetic / vector type, BSR_TB: blocks per tile.
// nrep > 1 (congruent diagonal blocks, e.g. the 8 cubes of a structured decomposition): the tiles describe ONE diagonal block and are applied to nrep vector segments of
// rep_stride entries each.  The replicas of a tile are consecutive workgroups of ONE XCD (every 8th workgroup index), so the tile's matrix bytes leave HBM once and the other
// nrep - 1 readers find them in that XCD's L2: an eighth of the device copy, an eighth of the host conversion, and a product that no longer streams 8 copies of K.
template <typename TM, typename T, int EPI, int BSR_TB>
__global__ __launch_bounds__(PMH_BLOCK) void k_bsr3(const int4 *__restrict__ tile_meta, const long long *__restrict__ tile_off, int ntiles, const int *__restrict__ browptr, const int *__restrict__ bcol, const TM *__restrict__ val, T scale,
                                                     const T *__restrict__ x, T *__restrict__ y, pmh_bsr3_epi<T> e, const int *__restrict__ halt, int nrep, long long rep_stride)
{
  constexpr int W = bsr_w<TM>;
  typedef TM    VM __attribute__((ext_vector_type(W)));
  typedef int   VI __attribute__((ext_vector_type(W)));
  __shared__ T prod[3][BSR_TB];
  const int    tid   = threadIdx.x;
  const int    chunk = (gridDim.x >> 3) / nrep; // XCD-aware: XCD x works on a contiguous slab of tiles (x stays in its L2), every tile for its nrep replicas in a row
  const int    v_    = blockIdx.x >> 3;
  const int    t     = (blockIdx.x & 7) * chunk + v_ / nrep;
  if (t >= ntiles) return;
  if (nrep > 1) {
    const long long o = (long long)(v_ % nrep) * rep_stride;
    x += o, y += o;
    if (e.y1) e.y1 += o;
    if (e.dinv) e.dinv += o;
    if (e.r) e.r += o;
    if (e.d) e.d += o;
    if (e.z64) e.z64 += o;
  }
  // the halt flag, the tile descriptor {first block row, end block row, first block, block count} and the tile's offset are
  // fetched together: one memory round trip instead of three dependent ones (the coarse-level launches are latency bound)
  const int       hlt = halt ? *halt : 0;
  const int4      tm  = tile_meta[t];
  const long long off = tile_off[t];
  if (hlt) return;
  const int br0 = tm.x, br1 = tm.y, s0 = tm.z, nbt = tm.w, nbp = (nbt + W - 1) / W * W;
  const TM       *v  = val + off * 9;
  const int      *bc = bcol + off;
#pragma unroll
  for (int jj = 0; jj < (BSR_TB / (PMH_BLOCK * W) > 0 ? BSR_TB / (PMH_BLOCK * W) : 1); jj++) {
    const int j0 = (tid + jj * PMH_BLOCK) * W;
    if (j0 < nbp) {
      const VI c = __builtin_nontemporal_load((const VI *)(bc + j0));
      VM       a[9];
#pragma unroll
      for (int k = 0; k < 9; k++) a[k] = __builtin_nontemporal_load((const VM *)(v + (size_t)k * nbp + j0));
#pragma unroll
      for (int w = 0; w < W; w++) {
        const int cw = c[w];
        const T   x0 = x[3 * cw], x1 = x[3 * cw + 1], x2 = x[3 * cw + 2];
#define A_(k) ((T)a[k][w])
        prod[0][j0 + w] = A_(0) * x0 + A_(1) * x1 + A_(2) * x2;
        prod[1][j0 + w] = A_(3) * x0 + A_(4) * x1 + A_(5) * x2;
        prod[2][j0 + w] = A_(6) * x0 + A_(7) * x1 + A_(8) * x2;
#undef A_
      }
    }
  }
  __syncthreads();
  const int nrows = 3 * (br1 - br0), sub = tid >> 2, lane = tid & 3;
  for (int rb = 0; rb < nrows; rb += PMH_BLOCK / 4) { // uniform trip count for the shuffles
    const int q   = rb + sub;
    T         sum = (T)0;
    if (q < nrows) {
      const int br = br0 + q / 3, r = q % 3;
      const int k0 = browptr[br] - s0, k1 = browptr[br + 1] - s0;
      for (int k = k0 + lane; k < k1; k += 4) sum += prod[r][k];
    }
    sum += __shfl_down(sum, 2, 4);
    sum += __shfl_down(sum, 1, 4);
    if (q < nrows && lane == 0) {
      const int row = 3 * br0 + q;
      if (sizeof(TM) == 2) sum *= scale; // fp16 storage keeps A / scale
      if (EPI == PMH_EPI_NONE) y[row] = sum;
      if (EPI == PMH_EPI_ADD) y[row] = e.y1[row] + sum;
      if (EPI == PMH_EPI_SUB) y[row] = sum - e.y1[row];
      if (EPI == PMH_BSR_EPI_PRE) y[row] = e.c0 * x[row] + e.c2 * e.dinv[row] * (e.y1[row] - sum);
      if (EPI == PMH_BSR_EPI_POST1) {
        const T rr = e.dinv[row] * (e.y1[row] - sum), dd = e.c0 * rr;
        e.r[row] = rr;
        e.d[row] = dd;
        y[row]   = x[row] + dd;
      }
      if (EPI == PMH_BSR_EPI_POST2) {
        const T vv = y[row] + e.c1 * x[row] + e.c2 * (e.r[row] - e.dinv[row] * sum);
        y[row] = vv;
        if (e.z64) e.z64[row] = (double)vv;
      }
    }
  }
}

// Build from a resident CSR (downloaded once); *out = NULL without error when the matrix has no 3x3 block structure that
// fits the tile (n not a multiple of 3, or a block row with more blocks than a tile holds).
int pmh_bsr3_from_csr(pmh_csr A, int storage, pmh_bsr3 *out, int tile, int nrep_hint)
{
  PMH_ARG(A && out && (storage == PMH_BSR_F64 || storage == PMH_BSR_F32 || storage == PMH_BSR_F16));
  *out        = nullptr;
  pmh_ctx ctx = A->ctx;
  if (A->nrows != A->ncols || A->nrows % 3 || A->nrows == 0) return PMH_SUCCESS;
  static const bool no_share = getenv("PMH_BSR_NO_SHARE") != nullptr; // A/B: one device copy per diagonal block (the HBM-streaming form)
  int nrep = (nrep_hint > 1 && !no_share && A->nrows % nrep_hint == 0 && (A->nrows / nrep_hint) % 3 == 0 && A->nnz % nrep_hint == 0) ? nrep_hint : 1;
  const int        n_all = A->nrows;
  int              n = n_all / nrep, nbr = n / 3;
  const int        tb = tile == 512 ? 512 : 1024; // 1024 measured best on MI355X for every entry type (profiles/r01_bsr3_tune.txt)
  const int        W  = storage == PMH_BSR_F64 ? bsr_w<double> : storage == PMH_BSR_F32 ? bsr_w<float> : bsr_w<_Float16>;
  const bool       verbose = getenv("PMH_CONTACT_TIMING") != nullptr && A->nnz > 10000000;
  auto             tnow    = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  double           tlast   = tnow();
  auto             stage   = [&](const char *what) {
    if (!verbose) return;
    const double t = tnow();
    fprintf(stderr, "      pmh_bsr3_from_csr: %-40s %.3f s\n", what, t - tlast);
    tlast = t;
  };
  std::vector<int>    rp_own, ci_own;
  std::vector<double> va_own;
  const int          *rp = A->h_rowptr, *ci = A->h_col;
  const double       *va = A->h_val;
  if (!(rp && (A->nnz == 0 || (ci && va)))) { // no host copy lent by the caller: download
    rp_own.resize((size_t)n_all + 1), ci_own.resize((size_t)A->nnz), va_own.resize((size_t)A->nnz);
    PMH_CHK(pmh_memcpy_d2h(ctx, rp_own.data(), A->d_rowptr, sizeof(int) * rp_own.size()));
    if (A->nnz) {
      PMH_CHK(pmh_memcpy_d2h(ctx, ci_own.data(), A->d_col, sizeof(int) * ci_own.size()));
      PMH_CHK(pmh_memcpy_d2h(ctx, va_own.data(), A->d_val, sizeof(double) * va_own.size()));
    }
    rp = rp_own.data(), ci = ci_own.data(), va = va_own.data();
  }
  stage("host copy of the CSR arrays");
  if (nrep > 1) {
    // the caller says the matrix is block diagonal with nrep congruent blocks: believed only after every entry of the other blocks has been compared with block 0
    // (threads over the replicas' rows; a mismatch anywhere falls back to the unshared form)
    const long long nnzb = A->nnz / nrep;
    bool            same = rp[n] == nnzb;
    for (int r = 1; r < nrep && same; r++) same = (long long)rp[(size_t)r * n] == (long long)r * nnzb;
    if (same && A->congruent_nrep == nrep) {
      // compared before (another storage of the same matrix)
    } else if (same) {
      const int         ntc = std::max(1, pmh_host_threads());
      std::vector<char> bad(ntc, 0);
      auto              cmp = [&](int tt) {
        for (int r = 1; r < nrep && !bad[tt]; r++) {
          const int       *rpr = rp + (size_t)r * n;
          const long long  ko  = (long long)r * nnzb;
          const int        i0 = (int)((long long)n * tt / ntc), i1 = (int)((long long)n * (tt + 1) / ntc);
          for (int i = i0; i < i1 && !bad[tt]; i++) {
            if ((long long)rpr[i + 1] - ko != rp[i + 1]) bad[tt] = 1;
            else
              for (int k = rp[i]; k < rp[i + 1]; k++)
                if (ci[k + ko] - r * n != ci[k] || memcmp(&va[k + ko], &va[k], sizeof(double)) || ci[k] >= n) {
                  bad[tt] = 1;
                  break;
                }
          }
        }
      };
      std::vector<std::thread> th;
      for (int tt = 0; tt < ntc; tt++) th.emplace_back(cmp, tt);
      for (auto &x : th) x.join();
      for (char b : bad) same = same && !b;
    }
    if (!same) nrep = 1, n = n_all, nbr = n / 3;
    else A->congruent_nrep = nrep;
    stage(nrep > 1 ? "congruent diagonal blocks confirmed (one device copy serves all)" : "diagonal blocks differ: one device copy each");
  }
  const long long nnz_used = nrep > 1 ? A->nnz / nrep : A->nnz;
  // block structure: union of the block columns of the three rows of each block row (sorted)
  // (host threads over contiguous ranges of block rows: the fine level of configs[2] has 158 M non-zeros and is converted three times per set-up)
  std::vector<int> browptr((size_t)nbr + 1, 0), bcol;
  const int        nt = std::max(1, std::min({pmh_host_threads(), nbr / 4096 + 1}));
  {
    std::vector<std::vector<int>> tbc(nt);
    std::vector<char>             toobig(nt, 0);
    auto work = [&](int t) {
      std::vector<int> tmp;
      tbc[t].reserve((size_t)(nnz_used / 9 / nt) + 16);
      for (int br = (int)((long long)nbr * t / nt); br < (int)((long long)nbr * (t + 1) / nt); br++) {
        tmp.clear();
        for (int r = 0; r < 3; r++)
          for (int k = rp[3 * br + r]; k < rp[3 * br + r + 1]; k++) tmp.push_back(ci[k] / 3);
        std::sort(tmp.begin(), tmp.end());
        tmp.erase(std::unique(tmp.begin(), tmp.end()), tmp.end());
        if ((int)tmp.size() > tb) {
          toobig[t] = 1;
          return;
        }
        tbc[t].insert(tbc[t].end(), tmp.begin(), tmp.end());
        browptr[br + 1] = (int)tmp.size();
      }
    };
    std::vector<std::thread> th;
    for (int t = 0; t < nt; t++) th.emplace_back(work, t);
    for (auto &x : th) x.join();
    size_t tot = 0;
    for (int t = 0; t < nt; t++) {
      if (toobig[t]) return PMH_SUCCESS;
      tot += tbc[t].size();
    }
    if (tot > (size_t)0x7fffff00) return PMH_SUCCESS;
    bcol.reserve(tot + 16);
    for (int t = 0; t < nt; t++) bcol.insert(bcol.end(), tbc[t].begin(), tbc[t].end());
    for (int br = 0; br < nbr; br++) browptr[br + 1] += browptr[br];
  }
  const long long nblocks = (long long)bcol.size();
  if (nblocks * 9 > 2 * nnz_used + 64) return PMH_SUCCESS; // blocks mostly empty: the CSR kernel moves fewer bytes
  stage("block structure");
  // tiles of whole block rows
  std::vector<int> tile_br(1, 0);
  for (int br = 0, start = 0; br < nbr; br++) {
    if (browptr[br + 1] - browptr[start] > tb) {
      tile_br.push_back(br);
      start = br;
    }
    if (br == nbr - 1) tile_br.push_back(nbr);
  }
  const int              ntiles = (int)tile_br.size() - 1;
  std::vector<long long> tile_off((size_t)ntiles + 1, 0); // padded block offsets
  for (int t = 0; t < ntiles; t++) {
    const int nbt   = browptr[tile_br[t + 1]] - browptr[tile_br[t]];
    tile_off[t + 1] = tile_off[t] + (nbt + W - 1) / W * W;
  }
  const long long npad = tile_off[ntiles];
  // values, tile-wise structure of arrays; padding blocks are zero and point at block column 0
  // (1.3 GB for the fine level of configs[2]: left uninitialised here, every thread zeroes the planes of its own tiles -- a zero-filled std::vector
  // was 0.22 s of page faults on one thread)
  std::unique_ptr<double[]> bv_own(new double[(size_t)npad * 9 + 1]);
  std::unique_ptr<int[]>    bcp_own(new int[(size_t)npad + 1]);
  double *const             bv  = bv_own.get();
  int *const                bcp = bcp_own.get();
  const size_t              nbv = (size_t)npad * 9;
  double              amax = 0.0;
  std::vector<double> tamax(nt, 0.0);
  stage("tile table, zeroed value planes");
  auto fill = [&](int tt) {
  double amax = 0.0;
  for (int t = (int)((long long)ntiles * tt / nt); t < (int)((long long)ntiles * (tt + 1) / nt); t++) {
    const int s0 = browptr[tile_br[t]], nbt = browptr[tile_br[t + 1]] - s0, nbp = (nbt + W - 1) / W * W;
    double   *v  = bv + (size_t)tile_off[t] * 9;
    std::fill(v, v + (size_t)nbp * 9, 0.0);
    std::copy(bcol.begin() + s0, bcol.begin() + s0 + nbt, bcp + tile_off[t]);
    std::fill(bcp + tile_off[t] + nbt, bcp + tile_off[t] + nbp, 0);
    for (int br = tile_br[t]; br < tile_br[t + 1]; br++) {
      const int *bc = bcol.data() + browptr[br];
      const int  nb = browptr[br + 1] - browptr[br];
      for (int r = 0; r < 3; r++)
        for (int k = rp[3 * br + r]; k < rp[3 * br + r + 1]; k++) {
          const int  c = ci[k] / 3, cc = ci[k] % 3;
          const int *p = std::lower_bound(bc, bc + nb, c);
          const int  j = (int)(p - bc) + browptr[br] - s0;
          v[(size_t)(3 * r + cc) * nbp + j] += va[k];
          amax = std::max(amax, fabs(va[k]));
        }
    }
  }
  tamax[tt] = amax;
  };
  {
    std::vector<std::thread> th;
    for (int t = 0; t < nt; t++) th.emplace_back(fill, t);
    for (auto &x : th) x.join();
    for (int t = 0; t < nt; t++) amax = std::max(amax, tamax[t]);
  }
  stage("values into the tile planes");
  pmh_bsr3 B = new pmh_bsr3_s();
  B->ctx = ctx, B->n = n_all, B->nbr = nbr, B->ntiles = ntiles, B->nblocks = nblocks, B->npad = npad, B->storage = storage, B->tb = tb;
  B->nrep = nrep, B->rep_rows = n; // nbr, ntiles, nblocks, npad describe ONE replica
  B->scale   = 1.0;
  B->ev_used = 0, B->ev_on = 0, B->ev_seen = 0, B->ev_stride = 1;
  std::vector<int> tmeta((size_t)4 * ntiles);
  for (int t = 0; t < ntiles; t++) {
    tmeta[4 * t] = tile_br[t], tmeta[4 * t + 1] = tile_br[t + 1];
    tmeta[4 * t + 2] = browptr[tile_br[t]], tmeta[4 * t + 3] = browptr[tile_br[t + 1]] - browptr[tile_br[t]];
  }
  PMH_CHK(pmh_malloc(ctx, sizeof(int) * (tmeta.size() ? tmeta.size() : 4), (void **)&B->d_tile_br));
  PMH_CHK(pmh_malloc(ctx, sizeof(long long) * tile_off.size(), (void **)&B->d_tile_off));
  PMH_CHK(pmh_malloc(ctx, sizeof(int) * browptr.size(), (void **)&B->d_browptr));
  PMH_CHK(pmh_malloc(ctx, sizeof(int) * (size_t)(npad + 2), (void **)&B->d_bcol));
  PMH_CHK(pmh_memcpy_h2d(ctx, B->d_tile_br, tmeta.data(), sizeof(int) * tmeta.size())); // int4 per tile
  PMH_CHK(pmh_memcpy_h2d(ctx, B->d_tile_off, tile_off.data(), sizeof(long long) * tile_off.size()));
  PMH_CHK(pmh_memcpy_h2d(ctx, B->d_browptr, browptr.data(), sizeof(int) * browptr.size()));
  PMH_CHK(pmh_memcpy_h2d(ctx, B->d_bcol, bcp, sizeof(int) * (size_t)npad));
  auto threaded = [&](auto &&body) { // body(first, one-past-last) over [0, nbv) on the conversion threads
    std::vector<std::thread> th;
    for (int t = 0; t < nt; t++) th.emplace_back(body, nbv * (size_t)t / nt, nbv * (size_t)(t + 1) / nt);
    for (auto &x : th) x.join();
  };
  if (storage == PMH_BSR_F32) {
    std::unique_ptr<float[]> bf(new float[nbv + 1]);
    threaded([&](size_t i0, size_t i1) {
      for (size_t i = i0; i < i1; i++) bf[i] = (float)bv[i];
    });
    PMH_CHK(pmh_malloc(ctx, sizeof(float) * (nbv + 2), &B->d_val));
    PMH_CHK(pmh_memcpy_h2d(ctx, B->d_val, bf.get(), sizeof(float) * nbv));
  } else if (storage == PMH_BSR_F16) {
    // power-of-two scale that brings the largest entry to [1, 2): entries below 2^-24 of it flush to zero
    int ex = 0;
    if (amax > 0.0) frexp(amax, &ex);
    B->scale = amax > 0.0 ? ldexp(1.0, ex - 1) : 1.0; // (no entry at all: 1, not the 2^-1 of ex = 0)
    const double               sc = B->scale;
    std::unique_ptr<_Float16[]> bh(new _Float16[nbv + 1]);
    threaded([&](size_t i0, size_t i1) {
      for (size_t i = i0; i < i1; i++) bh[i] = (_Float16)(float)(bv[i] / sc);
    });
    PMH_CHK(pmh_malloc(ctx, sizeof(_Float16) * (nbv + 4), &B->d_val));
    PMH_CHK(pmh_memcpy_h2d(ctx, B->d_val, bh.get(), sizeof(_Float16) * nbv));
  } else {
    PMH_CHK(pmh_malloc(ctx, sizeof(double) * (nbv + 2), &B->d_val));
    PMH_CHK(pmh_memcpy_h2d(ctx, B->d_val, bv, sizeof(double) * nbv));
  }
  stage("value conversion + upload");
  *out = B;
  return PMH_SUCCESS;
}

int pmh_bsr3_destroy(pmh_bsr3 B)
{
  if (!B) return PMH_SUCCESS;
  pmh_free(B->ctx, B->d_tile_br);
  pmh_free(B->ctx, B->d_tile_off);
  pmh_free(B->ctx, B->d_browptr);
  pmh_free(B->ctx, B->d_bcol);
  pmh_free(B->ctx, B->d_val);
  for (auto e : B->ev) (void)hipEventDestroy(e);
  delete B;
  return PMH_SUCCESS;
}

// bytes one launch moves from HBM: values + one index per block, block-row pointers, x read once, y written once.  With congruent blocks sharing one device copy
// (nrep > 1) the matrix is streamed ONCE (the other nrep - 1 readers of a tile find it in their XCD's L2); the vectors of all replicas are streamed.
double pmh_bsr3_bytes(pmh_bsr3 B)
{
  const double wm = (B->storage == PMH_BSR_F64) ? 8.0 : (B->storage == PMH_BSR_F32 ? 4.0 : 2.0);
  const double wv = (B->storage == PMH_BSR_F64) ? 8.0 : 4.0;
  return ((double)B->nblocks * (9.0 * wm + 4.0) + 4.0 * (B->nbr + 1)) + 2.0 * wv * B->n;
}

// the figure of the block-diagonal product as SURVEY 8d counts it (every K_i once): nrep times the matrix bytes.  Not an HBM figure when nrep > 1.
double pmh_bsr3_bytes_blockdiag(pmh_bsr3 B)
{
  const double wv = (B->storage == PMH_BSR_F64) ? 8.0 : 4.0;
  return (double)B->nrep * (pmh_bsr3_bytes(B) - 2.0 * wv * B->n) + 2.0 * wv * B->n;
}

int pmh_bsr3_replicas(pmh_bsr3 B) { return B->nrep; }

template <typename TM, typename T, int TB>
static int bsr3_launch_tb(pmh_bsr3 B, const T *x, T *y, int epi, const pmh_bsr3_epi<T> &e, const int *halt)
{
  const dim3       grid((unsigned)(((B->ntiles + 7) / 8) * 8 * B->nrep)), blk(PMH_BLOCK);
  hipStream_t      st = B->ctx->stream;
  const int4      *tb = (const int4 *)B->d_tile_br;
  const int       *bp = B->d_browptr, *bc = B->d_bcol;
  const long long *to = B->d_tile_off;
  const TM        *v  = (const TM *)B->d_val;
  const T          sc = (T)B->scale;
#define BSR_LAUNCH(EPI) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_bsr3<TM, T, EPI, TB>), grid, blk, 0, st, tb, to, B->ntiles, bp, bc, v, sc, x, y, e, halt, B->nrep, (long long)B->rep_rows)
  switch (epi) {
  case PMH_EPI_NONE: BSR_LAUNCH(PMH_EPI_NONE); break;
  case PMH_EPI_ADD: BSR_LAUNCH(PMH_EPI_ADD); break;
  case PMH_EPI_SUB: BSR_LAUNCH(PMH_EPI_SUB); break;
  case PMH_BSR_EPI_PRE: BSR_LAUNCH(PMH_BSR_EPI_PRE); break;
  case PMH_BSR_EPI_POST1: BSR_LAUNCH(PMH_BSR_EPI_POST1); break;
  case PMH_BSR_EPI_POST2: BSR_LAUNCH(PMH_BSR_EPI_POST2); break;
  default: return pmh_set_error(PMH_ERR_ARG, "bsr3: unsupported epilogue %d", epi);
  }
  PMH_HIP(hipGetLastError());
  return PMH_SUCCESS;
}

template <typename TM, typename T>
static int bsr3_launch(pmh_bsr3 B, const T *x, T *y, int epi, const pmh_bsr3_epi<T> &e, const int *halt)
{
  hipStream_t st    = B->ctx->stream;
  // event pairs on every ev_stride-th launch (PMH_TIMING_STRIDE, default 1): each pair costs ~4 us of stream time, which a
  // benchmark's timed region should not pay on all of its ~130 launches per step
  const bool  timed = B->ev_on && (B->ev_seen++ % B->ev_stride == 0) && (size_t)(B->ev_used + 2) <= B->ev.size();
  if (timed) PMH_HIP(hipEventRecord(B->ev[B->ev_used], st));
  if (B->tb == 512) PMH_CHK((bsr3_launch_tb<TM, T, 512>(B, x, y, epi, e, halt)));
  else PMH_CHK((bsr3_launch_tb<TM, T, 1024>(B, x, y, epi, e, halt)));
  if (timed) {
    PMH_HIP(hipEventRecord(B->ev[B->ev_used + 1], st));
    // operands of the fused epilogue beyond y = A x (one vector = n entries of the arithmetic type):
    // ADD/SUB read y1; PRE reads dinv, b; POST1 reads dinv, b and writes r, d; POST2 re-reads y, reads r, dinv (+ the fp64 copy)
    const double vec = (double)sizeof(T) * B->n;
    double       ex  = 0.0;
    if (epi == PMH_EPI_ADD || epi == PMH_EPI_SUB) ex = vec;
    else if (epi == PMH_BSR_EPI_PRE) ex = 2.0 * vec;
    else if (epi == PMH_BSR_EPI_POST1) ex = 4.0 * vec;
    else if (epi == PMH_BSR_EPI_POST2) ex = 3.0 * vec + (e.z64 ? 8.0 * B->n : 0.0);
    if (B->ev_extra.size() < B->ev.size() / 2) B->ev_extra.resize(B->ev.size() / 2, 0.0);
    B->ev_extra[B->ev_used / 2] = ex;
    B->ev_used += 2;
  }
  return PMH_SUCCESS;
}

int pmh_bsr3_spmv_epi_f64(pmh_bsr3 B, const double *x, double *y, int epi, const pmh_bsr3_epi<double> &e, const int *halt)
{
  PMH_ARG(B && B->storage == PMH_BSR_F64);
  return bsr3_launch<double, double>(B, x, y, epi, e, halt);
}

int pmh_bsr3_spmv_epi_f32(pmh_bsr3 B, const float *x, float *y, int epi, const pmh_bsr3_epi<float> &e, const int *halt)
{
  PMH_ARG(B && B->storage != PMH_BSR_F64);
  if (B->storage == PMH_BSR_F16) return bsr3_launch<_Float16, float>(B, x, y, epi, e, halt);
  return bsr3_launch<float, float>(B, x, y, epi, e, halt);
}

int pmh_bsr3_spmv_f64(pmh_bsr3 B, const double *x, double *y, int epi, const double *y1, const int *halt)
{
  pmh_bsr3_epi<double> e;
  memset(&e, 0, sizeof(e));
  e.y1 = y1;
  return pmh_bsr3_spmv_epi_f64(B, x, y, epi, e, halt);
}

int pmh_bsr3_spmv_f32(pmh_bsr3 B, const float *x, float *y, int epi, const float *y1, const int *halt)
{
  pmh_bsr3_epi<float> e;
  memset(&e, 0, sizeof(e));
  e.y1 = y1;
  return pmh_bsr3_spmv_epi_f32(B, x, y, epi, e, halt);
}

// ---- test entries (tests/test_gpu_bsr3_paths.py): the conversion as mg.hip and feti.hip call it, what it laid out, and one launch with a given epilogue; nothing
// inside the solvers calls them ----
extern "C" int pmh_bsr3_test_create(pmh_csr A, int storage, int tile, int nrep_hint, void **B)
{
  PMH_ARG(A && B);
  pmh_bsr3 b = nullptr;
  *B         = nullptr;
  PMH_CHK(pmh_bsr3_from_csr(A, storage, &b, tile, nrep_hint));
  *B = b;
  return PMH_SUCCESS;
}

extern "C" int pmh_bsr3_test_info(void *B_, long long info[8], double *scale)
{
  pmh_bsr3 B = (pmh_bsr3)B_;
  PMH_ARG(B && info);
  info[0] = B->n, info[1] = B->nbr, info[2] = B->ntiles, info[3] = B->tb, info[4] = B->nrep, info[5] = B->nblocks, info[6] = B->npad;
  info[7] = B->storage == PMH_BSR_F64 ? bsr_w<double> : B->storage == PMH_BSR_F32 ? bsr_w<float> : bsr_w<_Float16>;
  if (scale) *scale = B->scale;
  return PMH_SUCCESS;
}

template <typename T>
static int bsr3_test_launch(pmh_bsr3 B, int epi, const void *x, void *y, const void *y1, const void *dinv, void *r, void *d, double *z64, double c0, double c1, double c2, const int *halt)
{
  pmh_bsr3_epi<T> e;
  memset(&e, 0, sizeof(e));
  e.y1 = (const T *)y1, e.dinv = (const T *)dinv, e.r = (T *)r, e.d = (T *)d, e.z64 = z64, e.c0 = (T)c0, e.c1 = (T)c1, e.c2 = (T)c2;
  if constexpr (sizeof(T) == 8) return pmh_bsr3_spmv_epi_f64(B, (const T *)x, (T *)y, epi, e, halt);
  else return pmh_bsr3_spmv_epi_f32(B, (const T *)x, (T *)y, epi, e, halt);
}

extern "C" int pmh_bsr3_test_mult_epi(void *B_, int epi, const void *x, void *y, const void *y1, const void *dinv, void *r, void *d, double *z64, double c0, double c1, double c2, int halt)
{
  pmh_bsr3 B = (pmh_bsr3)B_;
  PMH_ARG(B && x && y);
  PMH_ARG(epi == PMH_EPI_NONE || epi == PMH_EPI_ADD || epi == PMH_EPI_SUB || epi == PMH_BSR_EPI_PRE || epi == PMH_BSR_EPI_POST1 || epi == PMH_BSR_EPI_POST2);
  PMH_ARG(x != (const void *)y); // no variant may write the vector it gathers from
  PMH_ARG((epi != PMH_EPI_ADD && epi != PMH_EPI_SUB) || y1);
  PMH_ARG(epi != PMH_BSR_EPI_PRE || (y1 && dinv));
  PMH_ARG(epi != PMH_BSR_EPI_POST1 || (y1 && dinv && r && d && x != (const void *)r && x != (const void *)d));
  PMH_ARG(epi != PMH_BSR_EPI_POST2 || (dinv && r && x != (const void *)z64));
  pmh_ctx ctx    = B->ctx;
  int    *d_halt = nullptr;
  if (halt) {
    const int one = 1;
    PMH_CHK(pmh_malloc(ctx, sizeof(int), (void **)&d_halt));
    PMH_CHK(pmh_memcpy_h2d(ctx, d_halt, &one, sizeof(int)));
  }
  int rc = B->storage == PMH_BSR_F64 ? bsr3_test_launch<double>(B, epi, x, y, y1, dinv, r, d, z64, c0, c1, c2, d_halt) : bsr3_test_launch<float>(B, epi, x, y, y1, dinv, r, d, z64, c0, c1, c2, d_halt);
  if (!rc && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = pmh_set_error(PMH_ERR_HIP, "pmh_bsr3_test_mult_epi: stream synchronisation failed");
  if (d_halt) pmh_free(ctx, d_halt);
  return rc;
}

extern "C" int pmh_bsr3_test_destroy(void *B) { return pmh_bsr3_destroy((pmh_bsr3)B); }

int pmh_bsr3_timing_enable(pmh_bsr3 B, int max_launches)
{
  PMH_ARG(B && max_launches >= 0);
  PMH_HIP(hipStreamSynchronize(B->ctx->stream));
  while ((int)B->ev.size() < 2 * max_launches) {
    hipEvent_t e;
    PMH_HIP(hipEventCreate(&e));
    B->ev.push_back(e);
  }
  B->ev_used = 0, B->ev_seen = 0, B->ev_stride = 1;
  if (const char *e = getenv("PMH_TIMING_STRIDE")) B->ev_stride = std::max(1, atoi(e));
  B->ev_on   = max_launches > 0;
  return PMH_SUCCESS;
}

// Launches of a halted chain return at once (no work, no bytes) and are left out: anything below a quarter of the upper-quartile
// duration.  (Not of the longest: the first launch of a kernel in a process pays the code-object load and can be 10x a normal one.)
int pmh_bsr3_timing_get(pmh_bsr3 B, int *launches, double *total_ms, double *epilogue_bytes)
{
  PMH_ARG(B && launches && total_ms);
  PMH_HIP(hipStreamSynchronize(B->ctx->stream));
  std::vector<float> ms(B->ev_used / 2);
  for (int i = 0; i < B->ev_used / 2; i++) PMH_HIP(hipEventElapsedTime(&ms[i], B->ev[2 * i], B->ev[2 * i + 1]));
  float mx = 0.f;
  if (!ms.empty()) {
    std::vector<float> srt(ms);
    std::sort(srt.begin(), srt.end());
    mx = srt[(size_t)(0.75 * (double)(srt.size() - 1))];
  }
  *launches = 0, *total_ms = 0.0;
  double ex = 0.0;
  for (size_t i = 0; i < ms.size(); i++)
    if (ms[i] >= 0.25f * mx) (*launches)++, *total_ms += ms[i], ex += (i < B->ev_extra.size() ? B->ev_extra[i] : 0.0);
  if (epilogue_bytes) *epilogue_bytes = ex; // summed over the counted launches
  return PMH_SUCCESS;
}
