// The entry-partitioned segmented sum of svm_csr.hip as its kernels and the K-column scoring sweep of svm_multi.hip share it: the span length, the table of
// the spans' first segments with their shared pieces, and the range of segments a span owns.  The scheme itself is described at the head of svm_csr.hip.
#pragma once
#include <algorithm>

#include "pmh_internal.h"

#define SVC_SPAN 2048 // stored entries per workgroup: 8 per thread, 16 KiB of products in LDS (up to 8 workgroups per CU)

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

struct svc_tab { // per compressed array: the spans' first segments and their shared pieces
  int    *first = nullptr;
  double *head = nullptr, *tail = nullptr;
  int     nb = 0;
};
static inline int svc_nb(long long nent) { return (int)std::max<long long>(1, (nent + SVC_SPAN - 1) / SVC_SPAN); } // (no entries: one span, every segment sums to 0)

// first[b] of every span of the array (ptr: nseg + 1 offsets, device) and room for the shared pieces: ncol sums per span in head and in tail
int svc_tab_build(pmh_ctx ctx, int nseg, const int *ptr, long long nent, svc_tab *t, int ncol = 1);
int svc_tab_free(pmh_ctx ctx, svc_tab *t);
