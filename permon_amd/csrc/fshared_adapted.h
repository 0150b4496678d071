// Orbit storage applied in the cube group's symmetry-adapted basis (included by fshared.hip only; the basis itself: orbitbasis.hip).
//
// W_c commutes with the 48 signed coordinate permutations, so in the basis U of orbitbasis.hip  U' W_c U = (+)_i (W^_i (x) I_{d_i})  over the ten irreps:
//     Y = U (+)_i (W^_i X^_i),  X^ = U' X,
// three launches: the forward transform (per orbit a 48 x 48 table times the orbit's rows of the multivector), k_fxa_prod (all ten blocks, one work table) and
// the inverse transform, which writes Y where k_fxo_fin writes it.  The transforms are k_fxa_narrow<false / true> for a multivector of at most 16 columns (the
// headline's 8; chosen once per class by fxa_build_class, launched by fxa_launch_transform) and k_fxa_transform<false / true>, shaped for 64 columns per workgroup,
// for wider ones (configs[3]); both sum every output in the same order, so the choice changes no bit.  X^ is written by the forward transform from the +x copies of
// X2, which the chain's gather (k_dc_gather) fills one launch earlier.  The blocks hold sum m_i^2 entries -- as many bytes as the orbit GEMM's A -- and are read ONCE
// per application for 8 d_i right-hand sides per group: about 5 flop per byte, a memory stream where the GEMM was compute-bound.
//
// Operand layouts (v_mfma_f64_16x16x4_f64: A[m = l & 15][k = l >> 4], B[k = l >> 4][n = l & 15], D column l & 15, rows (l >> 4) + 4 r):
//   Wh  block of 16 output rows ob, k step ks (8 columns of W^_i): 64 lanes x 2 doubles, lane l holds W^[16 ob + (l & 15)][8 ks + (l >> 4) + 4 h], h = 0, 1
//       -- a wave streams its 16 rows as contiguous 1 KB pieces with 16-byte loads; rows and columns past m are zero
//   Xh  block of 16 columns nb, k step ks: lane l holds X^[8 ks + (l >> 4) + 4 h][16 nb + (l & 15)]; column n = (partner * groups + group) * 8 + slot
//   Yh  row-major, ldy = 16 nbt doubles per row
// Every output row is summed inside ONE workgroup in a fixed order: no partial tiles in memory, no atomics, bitwise reproducible.
#pragma once
#include "fshared_kernels.h"

#define FXA_CB 64    // columns of the multivector per workgroup of the transforms
#define FXA_LDT 49   // row length of an orbit's table in LDS

__host__ __device__ __forceinline__ long long fxa_xh_off(const fxa_irrep &I, int r, int n) { return I.hoff + ((((long long)(n >> 4) * I.nks + (r >> 3)) * 64 + (r & 3) * 16 + (n & 15)) << 1) + ((r >> 2) & 1); }
__device__ __forceinline__ long long fxa_wh_off(const fxa_irrep &I, int r, int c) { return I.woff + ((((long long)(r >> 4) * I.nks + (c >> 3)) * 64 + (c & 3) * 16 + (r & 15)) << 1) + ((c >> 2) & 1); }

// One workgroup per (orbit, block of 64 columns); every orbit's table is stored as 48 x 48 (zero past the orbit's size).  rowinfo per basis function: irrep | partner << 4 | row of W^_irrep << 8.
// INV = false: X^ = U' X from the +x copies of the signed multivector X2; INV = true: Y = U Y^, written for the (position, slot) pairs some block touches (tmask)
template <bool INV>
__global__ __launch_bounds__(PMH_BLOCK) void k_fxa_transform(const fxa_irrep *__restrict__ ir, const double *__restrict__ tab, const long long *__restrict__ toff, const int *__restrict__ osize,
                                                             const int *__restrict__ tbase, const int *__restrict__ opos, const int *__restrict__ rowinfo, int NC, int nc, int ld, long long xbase0,
                                                             const double *__restrict__ X2, double *__restrict__ Xh, const double *__restrict__ Yh, double *__restrict__ Y,
                                                             const char *__restrict__ tmask)
{
  __shared__ double Ts[48 * FXA_LDT];
  __shared__ double vs[48 * FXA_CB];
  const int o = blockIdx.x, no = osize[o], tb = tbase[o], c0 = blockIdx.y * FXA_CB, ncb = min(FXA_CB, NC - c0);
  const double *__restrict__ T = tab + toff[o]; // 48 x 48, zero past the orbit's size
  for (int e = threadIdx.x; e < 48 * 48; e += PMH_BLOCK) {
    const int t = e / 48, j = e % 48;
    Ts[INV ? j * FXA_LDT + t : t * FXA_LDT + j] = T[e];
  }
  for (int e = threadIdx.x; e < ((no + 3) & ~3) * ncb; e += PMH_BLOCK) {
    const int b = e / ncb, cl = e % ncb, col = c0 + cl;
    if (b >= no) vs[b * FXA_CB + cl] = 0.0; // (the sums below run in fours)
    else if (INV) {
      const int       ri = rowinfo[tb + b];
      const fxa_irrep I  = ir[ri & 15];
      vs[b * FXA_CB + cl] = Yh[I.yoff + (long long)(ri >> 8) * I.ldy + ((ri >> 4) & 3) * NC + col];
    } else
      vs[b * FXA_CB + cl] = X2[2 * (xbase0 + (long long)(col >> 3) * ld * FXS_S + (long long)opos[tb + b] * FXS_S) + (col & 7)];
  }
  __syncthreads();
  for (int e = threadIdx.x; e < no * ncb; e += PMH_BLOCK) {
    const int a = e / ncb, cl = e % ncb, col = c0 + cl;
    // four interleaved partial sums (terms b = 0, 4, 8, ... and so on; the orbit sizes are multiples of 4), added in a fixed order: four LDS reads in flight
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    for (int b = 0; b < no; b += 4) {
      s0 = FXS_MAD(Ts[a * FXA_LDT + b], vs[b * FXA_CB + cl], s0), s1 = FXS_MAD(Ts[a * FXA_LDT + b + 1], vs[(b + 1) * FXA_CB + cl], s1);
      s2 = FXS_MAD(Ts[a * FXA_LDT + b + 2], vs[(b + 2) * FXA_CB + cl], s2), s3 = FXS_MAD(Ts[a * FXA_LDT + b + 3], vs[(b + 3) * FXA_CB + cl], s3);
    }
    const double s = (s0 + s1) + (s2 + s3);
    if (INV) {
      const int pos = opos[tb + a], g = col >> 3, sl = col & 7;
      if (tmask[((long long)g * nc + pos) * FXS_S + sl]) Y[xbase0 + (long long)g * ld * FXS_S + (long long)pos * FXS_S + sl] = s;
    } else {
      const int       ri = rowinfo[tb + a];
      const fxa_irrep I  = ir[ri & 15];
      Xh[fxa_xh_off(I, ri >> 8, ((ri >> 4) & 3) * NC + col)] = s;
    }
  }
}

// The transforms of a narrow multivector (NC <= FXN_NC: one or two groups of 8 slots; the headline has one).  One workgroup of 192 threads per (orbit, group of 8
// columns), one thread per (output row a, pair of slots): all 48 x 8 outputs in ONE round, nothing divided by a run-time number.  The thread reads ITS row of the table
// straight from memory with 16-byte loads -- the 4 lanes of a row share every load -- so no table is staged, transposed or indexed in LDS.  The set-up stores the
// tables for this kernel in the order its waves load them (fxn_tab_off: the k-th 16 bytes of a wave's 16 rows side by side, so one load instruction reads 256
// contiguous bytes, not 16 bytes out of each of 16 rows 384 bytes apart) and a second time transposed for the inverse direction; a launch reads one of the two
// copies.  LDS holds the orbit's operand block alone (3 KB), read 16 bytes at a time.
// A thread per (row, slot) was built first: its 48 table entries are 96 VGPRs whichever way the loads are placed (108 .. 114 in all, scratch under a tighter bound), 4
// waves per SIMD, and the headline's 715 orbits x 6 waves then do not fit the chip at once; with two slots per thread the same registers feed two outputs and 715 x 3
// waves do.  Every look-up chain of k_fxa_transform is a record per basis function, built by fxa_build_class (orbits padded to 48 functions,
// f = (group * orbits + orbit) * 48 + a):
//   forward  rec[orbit * 48 + a] = 16 * position: the +x copy in the group's part of X2;  recl[f] = fxa_xh_off of the function's row for slot 0 of the group (+ 2 per slot)
//   inverse  recl[f] = the function's entry of Y^ for slot 0 of the group (+ 1 per slot);  rec[f] = position << 8 | the 8 slots' tmask bits
// so both kernels have two dependent global loads in front of their sums (record -> operand; the table's row comes beside them) and none behind.
// The sums are k_fxa_transform's: per output four interleaved partial sums over b = 0, 4, 8, ..., each term by FXS_MAD, (s0 + s1) + (s2 + s3); the table's entries and
// the operands past the orbit's size are zero -- every output keeps its bits.
#define FXN_NC 16
#define FXN_T (48 * FXS_S / 2)
// entry (row a, column j) of an orbit's 48 x 48 table in k_fxa_narrow's copies: wave a >> 4, its 16-byte piece j >> 1, row a & 15 of the wave
__host__ __device__ __forceinline__ int fxn_tab_off(int a, int j) { return ((((a >> 4) * 24 + (j >> 1)) * 16 + (a & 15)) << 1) + (j & 1); }

template <bool INV>
__global__ __launch_bounds__(FXN_T) void k_fxa_narrow(const double *__restrict__ tab, const int *__restrict__ osize, const int *__restrict__ rec, const long long *__restrict__ recl, int norb,
                                                      long long gstride, const double *__restrict__ src, double *__restrict__ dst)
{
  __shared__ dbl2 vs[FXN_T];
  const int  o = blockIdx.x, g = blockIdx.y, a = threadIdx.x >> 2, sl = 2 * (threadIdx.x & 3), no = osize[o];
  const bool live = a < no;
  int        r  = 0;
  long long  rl = 0;
  dbl2       v  = dbl2{0.0, 0.0}, t[24];
#pragma unroll
  for (int k = 0; k < 24; k++) t[k] = dbl2{0.0, 0.0};
  if (live) {
    const long long f = ((long long)g * norb + o) * 48 + a;
    r = rec[INV ? f : o * 48 + a], rl = recl[f];
    const dbl2 *__restrict__ row = (const dbl2 *)(tab + (long long)o * 48 * 48 + fxn_tab_off(a, 0));
#pragma unroll
    for (int k = 0; k < 24; k++)
      if (2 * k < no) t[k] = row[16 * k];
    v = *(const dbl2 *)(INV ? src + rl + sl : src + (long long)g * gstride + r + sl);
  }
  vs[threadIdx.x] = v; // (rows past the orbit's size: zero, the sums below run in fours)
  __syncthreads();
  if (!live) return;
  dbl2 s0 = dbl2{0.0, 0.0}, s1 = s0, s2 = s0, s3 = s0; // .x: slot sl, .y: slot sl + 1
#pragma unroll
  for (int k = 0; k < 12; k++)
    if (4 * k < no) {
      const dbl2 *x = vs + 4 * k * (FXS_S / 2) + (threadIdx.x & 3);
      const dbl2  x0 = x[0], x1 = x[FXS_S / 2], x2 = x[2 * (FXS_S / 2)], x3 = x[3 * (FXS_S / 2)];
      s0.x = FXS_MAD(t[2 * k].x, x0.x, s0.x), s1.x = FXS_MAD(t[2 * k].y, x1.x, s1.x), s2.x = FXS_MAD(t[2 * k + 1].x, x2.x, s2.x), s3.x = FXS_MAD(t[2 * k + 1].y, x3.x, s3.x);
      s0.y = FXS_MAD(t[2 * k].x, x0.y, s0.y), s1.y = FXS_MAD(t[2 * k].y, x1.y, s1.y), s2.y = FXS_MAD(t[2 * k + 1].x, x2.y, s2.y), s3.y = FXS_MAD(t[2 * k + 1].y, x3.y, s3.y);
    }
  const double sx = (s0.x + s1.x) + (s2.x + s3.x), sy = (s0.y + s1.y) + (s2.y + s3.y);
  if (INV) {
    double *__restrict__ y = dst + (long long)g * gstride + (long long)(r >> 8) * FXS_S + sl;
    if ((r >> sl) & 1) y[0] = sx;
    if ((r >> sl) & 2) y[1] = sy;
  } else
    dst[rl + 2 * sl] = sx, dst[rl + 2 * sl + 2] = sy;
}

// tests (pmh_fexplicit_orbit_adapted_transform): X^ / Y^ in the order (basis function, column) <-> the operand layouts
template <bool TOYH>
__global__ __launch_bounds__(PMH_BLOCK) void k_fxa_logical(const fxa_irrep *__restrict__ ir, const int *__restrict__ rowinfo, int nc, int NC, const double *__restrict__ in, double *__restrict__ out)
{
  const long long e = (long long)blockIdx.x * PMH_BLOCK + threadIdx.x;
  if (e >= (long long)nc * NC) return;
  const int       ri = rowinfo[e / NC], col = (int)(e % NC), n = ((ri >> 4) & 3) * NC + col;
  const fxa_irrep I  = ir[ri & 15];
  if (TOYH) out[I.yoff + (long long)(ri >> 8) * I.ldy + n] = in[e];
  else out[e] = in[fxa_xh_off(I, ri >> 8, n)];
}

// 16 rows of Y^_i = W^_i X^_i on NBW blocks of 16 columns.  The four waves of the workgroup share the k range (whole trips of U k steps, fxa_wave_k0: U KB of W^ and
// U NBW KB of X^, which stays in the caches, in flight per wave), so that a row block's sum is a chain of a quarter of the products and the chip holds several waves
// per SIMD to cover the loads' latency; wave 0 adds the other waves' sums in wave order and stores: still ONE fixed order per output entry.
// W^ is read with plain loads, not with the non-temporal hint: the blocks are the same bytes at every application and little else is read between two of them, so
// part of them is still in the last-level cache when the next application comes (the hint kept them out of it).  This rests on ONE class whose blocks (190 MB on the
// headline) are smaller than that cache (256 MB): blocks larger than it, or several classes applied in turn, would sweep it for nothing and push the chain's vectors
// out (its small kernels already take 1 .. 4 us longer beside the 190 MB).  Neither was measured; the hint would then have to be chosen by the blocks' size at set-up.
template <int NBW, int U>
__device__ __forceinline__ void fxa_prod_rows(const fxa_irrep &I, int ob, int nb0, const double *__restrict__ Wh, const double *__restrict__ Xh, double *__restrict__ Yh, int lane, int wave,
                                              double (*red)[16 * 64])
{
  const dbl2 *__restrict__ w = (const dbl2 *)(Wh + I.woff + (long long)ob * I.nks * 128) + lane;
  const dbl2 *__restrict__ x = (const dbl2 *)(Xh + I.hoff + (long long)nb0 * I.nks * 128) + lane;
  dbl4 acc[NBW];
#pragma unroll
  for (int j = 0; j < NBW; j++) acc[j] = dbl4{0.0, 0.0, 0.0, 0.0};
  const int ks1 = fxa_wave_k0(I.nks, U, wave + 1);
  for (int ks = fxa_wave_k0(I.nks, U, wave); ks < ks1; ks += U) {
    dbl2 a[U], b[U][NBW];
#pragma unroll
    for (int u = 0; u < U; u++) a[u] = w[(long long)(ks + u) * 64];
#pragma unroll
    for (int u = 0; u < U; u++)
#pragma unroll
      for (int j = 0; j < NBW; j++) b[u][j] = x[((long long)j * I.nks + ks + u) * 64];
#pragma unroll
    for (int u = 0; u < U; u++) {
#pragma unroll
      for (int j = 0; j < NBW; j++) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u].x, b[u][j].x, acc[j], 0, 0, 0);
#pragma unroll
      for (int j = 0; j < NBW; j++) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u].y, b[u][j].y, acc[j], 0, 0, 0);
    }
  }
  if (wave > 0) {
#pragma unroll
    for (int j = 0; j < NBW; j++)
#pragma unroll
      for (int r = 0; r < 4; r++) red[wave - 1][(4 * j + r) * 64 + lane] = acc[j][r];
  }
  __syncthreads();
  if (wave > 0) return;
#pragma unroll
  for (int v = 0; v < FXA_WAVES - 1; v++)
#pragma unroll
    for (int j = 0; j < NBW; j++)
#pragma unroll
      for (int r = 0; r < 4; r++) acc[j][r] += red[v][(4 * j + r) * 64 + lane];
  double *__restrict__ y = Yh + I.yoff + (long long)(ob * 16 + (lane >> 4)) * I.ldy + nb0 * 16 + (lane & 15);
#pragma unroll
  for (int j = 0; j < NBW; j++)
#pragma unroll
    for (int r = 0; r < 4; r++) y[(long long)(4 * r) * I.ldy + j * 16] = acc[j][r];
}

// items: (irrep, block of 16 output rows, first block of 16 columns, blocks of columns 1 .. 4), the longest first
__global__ __launch_bounds__(64 * FXA_WAVES) void k_fxa_prod(const int *__restrict__ items, const fxa_irrep *__restrict__ ir, const double *__restrict__ Wh, const double *__restrict__ Xh,
                                                              double *__restrict__ Yh)
{
  __shared__ double red[FXA_WAVES - 1][16 * 64];
  const int *it = items + 4 * blockIdx.x;
  const int  lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const fxa_irrep I = ir[__builtin_amdgcn_readfirstlane(it[0])];
  const int  ob = __builtin_amdgcn_readfirstlane(it[1]), nb0 = __builtin_amdgcn_readfirstlane(it[2]), nbw = __builtin_amdgcn_readfirstlane(it[3]);
  switch (nbw) {
  case 1: fxa_prod_rows<1, fxa_trip_steps(1)>(I, ob, nb0, Wh, Xh, Yh, lane, wave, red); break;
  case 2: fxa_prod_rows<2, fxa_trip_steps(2)>(I, ob, nb0, Wh, Xh, Yh, lane, wave, red); break;
  case 3: fxa_prod_rows<3, fxa_trip_steps(3)>(I, ob, nb0, Wh, Xh, Yh, lane, wave, red); break;
  default: fxa_prod_rows<4, fxa_trip_steps(4)>(I, ob, nb0, Wh, Xh, Yh, lane, wave, red); break;
  }
}

// ---- set-up.  The blocks are built from the representatives' rows alone, which presumes that W_c is invariant EXACTLY.  A representative p fixed by a stabiliser H
// has a row that should satisfy W[p][c] = s_h(p) s_h(c) W[p][h c] for h in H, and does so only as far as its K^+ solve converged: the row is replaced by its average
// over H (step 0; the exact row is a fixed point), so that the matrix the GEMM rebuilds by symmetry and the one the blocks stand for are the same to rounding.
__global__ __launch_bounds__(PMH_BLOCK) void k_fxa_stab_avg(int nh, const int *__restrict__ hops, int p, int pr, int tm, int nc, int nkc, const int *__restrict__ posmap, const signed char *__restrict__ sign,
                                                             const int *__restrict__ kinv, const double *__restrict__ A, double *__restrict__ tmp)
{
  const double *__restrict__ arow = A + (long long)(pr / tm) * nkc * (FXO_TK * tm) + pr % tm;
  for (int c = blockIdx.x * PMH_BLOCK + threadIdx.x; c < nc; c += gridDim.x * PMH_BLOCK) {
    double s = 0.0;
    for (int h = 0; h < nh; h++) {
      const int g = hops[h], k = kinv[posmap[(long long)g * nc + c]];
      s += (double)(sign[(long long)g * nc + p] * sign[(long long)g * nc + c]) * arow[(long long)(k / FXO_TK) * (FXO_TK * tm) + (k % FXO_TK) * tm];
    }
    tmp[c] = s / nh;
  }
}
__global__ __launch_bounds__(PMH_BLOCK) void k_fxa_stab_store(int pr, int tm, int nc, int nkc, const int *__restrict__ kinv, const double *__restrict__ tmp, double *__restrict__ A)
{
  double *__restrict__ arow = A + (long long)(pr / tm) * nkc * (FXO_TK * tm) + pr % tm;
  for (int c = blockIdx.x * PMH_BLOCK + threadIdx.x; c < nc; c += gridDim.x * PMH_BLOCK) {
    const int k = kinv[c];
    arow[(long long)(k / FXO_TK) * (FXO_TK * tm) + (k % FXO_TK) * tm] = tmp[c];
  }
}

// W^_i[(P, k), (C, l)] = sqrt(|O_P| / d_i) sum_b (v_{P,k})_b A^_p[(C, l, b)],  A^_p = the forward transform of the representative's row of A
// step 1: Abuf[basis function][orbit P] = sum_j table[function][j] A[row of P's representative][position j of the function's orbit]; grid (orbits, M / 64)
__global__ __launch_bounds__(64) void k_fxa_rows(int M, int tm, int nkc, const double *__restrict__ tab, const long long *__restrict__ toff, const int *__restrict__ osize, const int *__restrict__ tbase,
                                                 const int *__restrict__ opos, const int *__restrict__ kinv, const int *__restrict__ reprow, const double *__restrict__ A, double *__restrict__ Abuf)
{
  __shared__ double as[48][64];
  const int o = blockIdx.x, no = osize[o], tb = tbase[o], P = blockIdx.y * 64 + threadIdx.x;
  const bool in = P < M;
  const int  pr = in ? reprow[P] : 0;
  const double *__restrict__ arow = A + (long long)(pr / tm) * nkc * (FXO_TK * tm) + pr % tm;
  for (int j = 0; j < no; j++) {
    const int k = kinv[opos[tb + j]];
    as[j][threadIdx.x] = in ? arow[(long long)(k / FXO_TK) * (FXO_TK * tm) + (k % FXO_TK) * tm] : 0.0;
  }
  const double *__restrict__ T = tab + toff[o];
  for (int t = 0; t < no; t++) {
    double s = 0.0;
    for (int j = 0; j < no; j++) s = FXS_MAD(T[t * 48 + j], as[j][threadIdx.x], s);
    if (in) Abuf[(long long)(tb + t) * M + P] = s;
  }
}

// step 2, per irrep: entry (r, c) of W^_i into the operand layout.  fn0[c]: the basis function (partner 0) of column c's copy; orb[r], vs[3 r ...]: the orbit of
// row r's copy and its vector times sqrt(|O| / d)
__global__ __launch_bounds__(PMH_BLOCK) void k_fxa_combine(fxa_irrep I, int M, const int *__restrict__ fn0, const int *__restrict__ orb, const double *__restrict__ vs, const double *__restrict__ Abuf,
                                                            double *__restrict__ Wh)
{
  const long long e = (long long)blockIdx.x * PMH_BLOCK + threadIdx.x;
  if (e >= (long long)I.m * I.m) return;
  const int r = (int)(e / I.m), c = (int)(e % I.m);
  double    s = 0.0;
  for (int b = 0; b < I.d; b++) s = FXS_MAD(vs[3 * r + b], Abuf[(long long)(fn0[c] + b) * M + orb[r]], s);
  Wh[fxa_wh_off(I, r, c)] = s;
}
