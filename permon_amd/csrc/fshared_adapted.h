// Orbit storage applied in the cube group's symmetry-adapted basis (included by fshared.hip only; the basis itself: orbitbasis.hip).
//
// W_c commutes with the 48 signed coordinate permutations, so in the basis U of orbitbasis.hip  U' W_c U = (+)_i (W^_i (x) I_{d_i})  over the ten irreps:
//     Y = U (+)_i (W^_i X^_i),  X^ = U' X,
// three launches: k_fxa_transform<false> (per orbit a 48 x 48 table times the orbit's rows of the multivector), k_fxa_prod (all ten blocks, one work table) and
// k_fxa_transform<true>, which writes Y where k_fxo_fin writes it.  The blocks hold sum m_i^2 entries -- as many bytes as the orbit GEMM's A -- and are read ONCE
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

__device__ __forceinline__ long long fxa_xh_off(const fxa_irrep &I, int r, int n) { return I.hoff + ((((long long)(n >> 4) * I.nks + (r >> 3)) * 64 + (r & 3) * 16 + (n & 15)) << 1) + ((r >> 2) & 1); }
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
