// The entry-partitioned segmented sum, written once for its two users: the kernels of svm_csr.hip (one sum per segment) and the K-column scoring sweep of
// svm_multi.hip (KC sums per segment).  The scheme itself is described at the head of svm_csr.hip.  Here: the span length, the table of the spans' first
// segments with their shared pieces, the guarded span load, the per-segment body (svc_segments) and the finishing body (svc_finish).  A kernel stages its
// span in LDS its own way and says with two functors what an entry adds to the sums (term) and what becomes of a finished segment (done).
#pragma once
#include <algorithm>

#include "svm_rows.h"

#define SVC_SPAN 2048 // stored entries per workgroup: 8 per thread, 16 KiB of products in LDS (up to 8 workgroups per CU)

typedef int int2v __attribute__((ext_vector_type(2))); // (beside dbl2 of svm_rows.h)

// slot j of this thread's share of the span [start, end): the entries k, k + 1 with k = start + 2 (j PMH_BLOCK + threadIdx.x), by one 16-byte value and one
// 8-byte index load (start is even and the arrays are 16-byte aligned); entries past the end: 0, column 0
static __device__ __forceinline__ void svc_load_pair(int j, int start, int end, const double *__restrict__ val, const int *__restrict__ idx, dbl2 &v, int2v &ix)
{
  const int k = start + 2 * (j * PMH_BLOCK + (int)threadIdx.x);
  v = dbl2{0.0, 0.0}, ix = int2v{0, 0};
  if (k + 1 < end) {
    v  = __builtin_nontemporal_load((const dbl2 *)(val + k));
    ix = __builtin_nontemporal_load((const int2v *)(idx + k));
  } else if (k < end) v.x = val[k], ix.x = idx[k];
}

// the segments of span b: c0 .. c1.  A segment that ends exactly at the span's end is the span's; empty segments at that boundary too
static __device__ __forceinline__ void svc_range(int b, int nb, int nseg, int end, const int *__restrict__ ptr, const int *__restrict__ first, int &c0, int &c1)
{
  c0 = first[b];
  c1 = nseg - 1;
  if (b + 1 < nb) {
    const int cf = first[b + 1];
    c1           = ptr[cf] == end ? cf - 1 : cf;
  }
}

// Span b = [start, end), staged by the caller: the KC sums of every segment's piece inside the span.  term(k, s) adds the span's entry k (0 .. SVC_SPAN) to
// s[0 .. KC); a piece's G lanes take its entries lo + l, lo + l + G, .. ascending, then the shfl_down tree G/2 .. 1.  done(c, s) receives a segment that lies
// whole in the span; the at most two shared pieces go to head / tail (KC doubles per span)
template <int KC, class T, class D>
static __device__ __forceinline__ void svc_segments(int b, int nb, int nseg, int start, int end, const int *__restrict__ ptr, const int *__restrict__ first, double *__restrict__ head,
                                                    double *__restrict__ tail, T term, D done)
{
  int c0, c1;
  svc_range(b, nb, nseg, end, ptr, first, c0, c1);
  // lanes per segment: the largest power of two <= mean piece length / 4, at most a wavefront
  const int avg = (end - start) / (c1 - c0 + 1);
  int       G   = 1;
  while (G < 64 && G * 8 <= avg) G <<= 1;
  const int g = threadIdx.x / G, l = threadIdx.x % G;
  for (int c = c0 + g; c <= c1; c += PMH_BLOCK / G) { // (the trip count is uniform over a segment's G lanes)
    const int p0 = ptr[c], p1 = ptr[c + 1], lo = max(p0, start) - start, hi = min(p1, end) - start;
    double    s[KC];
#pragma unroll
    for (int j = 0; j < KC; j++) s[j] = 0.0;
    for (int k = lo + l; k < hi; k += G) term(k, s);
    for (int w = G >> 1; w > 0; w >>= 1)
#pragma unroll
      for (int j = 0; j < KC; j++) s[j] += __shfl_down(s[j], w, G);
    if (l == 0) {
      if (p0 >= start && p1 <= end) done(c, s); // the whole segment lies in this span
      else {
        double *dst = (c == c0 ? head : tail) + (size_t)b * KC;
#pragma unroll
        for (int j = 0; j < KC; j++) dst[j] = s[j];
      }
    }
  }
}

// One wavefront per span: where the span's first segment began in an earlier span and ends in this one, add its pieces in span order (lane l takes the spans
// b0 + l, b0 + l + 64, ..), then pmh_wave_sum per column, and done(c, s) in lane 0
template <int KC, class D>
static __device__ __forceinline__ void svc_finish(int nent, int nseg, int nb, const int *__restrict__ ptr, const int *__restrict__ first, const double *__restrict__ head,
                                                  const double *__restrict__ tail, D done)
{
  const int lane = threadIdx.x & 63, b = blockIdx.x * (PMH_BLOCK / 64) + (threadIdx.x >> 6);
  if (b >= nb) return;
  const int start = b * SVC_SPAN, end = min(start + SVC_SPAN, nent), c = first[b], p0 = ptr[c], p1 = ptr[c + 1];
  if (!(p0 < start && p1 <= end)) return; // (wave-uniform)
  const int  b0    = p0 / SVC_SPAN;
  const bool tail0 = first[b0] != c; // in the span where it begins the segment is the last of several: its piece is that span's tail
  double     s[KC];
#pragma unroll
  for (int j = 0; j < KC; j++) s[j] = 0.0;
  for (int bb = b0 + lane; bb <= b; bb += 64) {
    const double *p = ((bb == b0 && tail0) ? tail : head) + (size_t)bb * KC;
#pragma unroll
    for (int j = 0; j < KC; j++) s[j] += p[j];
  }
#pragma unroll
  for (int j = 0; j < KC; j++) s[j] = pmh_wave_sum(s[j]);
  if (lane == 0) done(c, s);
}

struct svc_tab { // per compressed array: the spans' first segments and their shared pieces
  int    *first = nullptr;
  double *head = nullptr, *tail = nullptr;
  int     nb = 0;
};
static inline int svc_nb(long long nent) { return (int)std::max<long long>(1, (nent + SVC_SPAN - 1) / SVC_SPAN); } // (no entries: one span, every segment sums to 0)

// first[b] of every span of the array (ptr: nseg + 1 offsets, device) and room for the shared pieces: ncol sums per span in head and in tail
int svc_tab_build(pmh_ctx ctx, int nseg, const int *ptr, long long nent, svc_tab *t, int ncol = 1);
int svc_tab_free(pmh_ctx ctx, svc_tab *t);
