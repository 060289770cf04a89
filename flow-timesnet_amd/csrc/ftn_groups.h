// The CSR of the series groups (include/flowtimes.h, ftn_group_sum), stated once for k_group_sum and k_group_sum_rows:
// what the entries check about the host copy, and how the device copy is read - a walk in plain C++ without HIP, which
// tests/test_groups_csr_host.py runs in a stand-alone program under the host sanitizers.  The device words are not
// validated; the host copy is, and it sizes the launch (C chunks).  Offsets are clamped to 0 .. M and cfirst to 0 .. C
// where it is written, so whatever the device words are, cfirst rises from 0 within 0 .. C, a combine range
// cfirst[g] .. cfirst[g + 1] lies inside C chunk sums, and a chunk c < C reads `order` inside 0 .. M (ftn_csr_chunk).
// Where they agree with the host copy every clamp is the identity.  Counts fit int: M <= 32 C <= 65536, chunks <= G C.
#pragma once
#include "../../include/flowtimes.h"
#ifdef __HIPCC__
#include "ftn_common.h"
#define FTN_CSR_FN __host__ __device__ __forceinline__
#else
#define FTN_CSR_FN static inline
#endif

struct FtnGroupCsr {
  const int *order, *offsets;   // device: [M] members, [G + 1] offsets
  int G, M, C;                  // groups, members, and the chunks of the validated host offsets
};

FTN_CSR_FN int ftn_csr_offset(const FtnGroupCsr& s, int g) {
  const int o = s.offsets[g];
  return o < 0 ? 0 : o > s.M ? s.M : o;
}
FTN_CSR_FN int ftn_csr_chunks(const FtnGroupCsr& s, int g) {
  const int m = ftn_csr_offset(s, g + 1) - ftn_csr_offset(s, g);
  return m > 0 ? (m + FTN_GROUP_CHUNK - 1) / FTN_GROUP_CHUNK : 0;
}

// cfirst [G + 1], the first chunk of every group: a prefix sum by `nthreads` threads, thread t taking the `per`
// consecutive groups g0 .. g1 - 1.  Before a barrier it leaves their chunks in part[t] (ftn_csr_count); after it, it
// writes their cfirst, and the last thread cfirst[G] (ftn_csr_first).
FTN_CSR_FN int ftn_csr_count(const FtnGroupCsr& s, int t, int nthreads, int* g0, int* g1) {
  const int per = (s.G + nthreads - 1) / nthreads;
  *g0 = t * per < s.G ? t * per : s.G;
  *g1 = *g0 + per < s.G ? *g0 + per : s.G;
  int n = 0;
  for (int g = *g0; g < *g1; ++g) n += ftn_csr_chunks(s, g);
  return n;
}
FTN_CSR_FN void ftn_csr_first(const FtnGroupCsr& s, int t, int nthreads, int g0, int g1, const int* part, int* cfirst) {
  int base = 0;
  for (int u = 0; u < t; ++u) base += part[u];
  for (int g = g0; g < g1; ++g) {
    cfirst[g] = base < s.C ? base : s.C;
    base += ftn_csr_chunks(s, g);
  }
  if (t == nthreads - 1) cfirst[s.G] = base < s.C ? base : s.C;
}

// Chunk c in 0 .. C - 1 -> its group g and its members order[start + j], 0 <= j < min(len, FTN_GROUP_CHUNK).  g is the
// last group with cfirst[g] <= c (cfirst[0] = 0).  Below the clamp cfirst is the true prefix sum, so when a later group
// begins past c, c is one of g's chunks: 0 < len, start + len <= M.  Else g = G - 1, and a c past its chunks has len <= 0.
struct FtnGroupChunk { int g, start, len; };
FTN_CSR_FN FtnGroupChunk ftn_csr_chunk(const FtnGroupCsr& s, const int* cfirst, int c) {
  int lo = 0, hi = s.G;                                         // the first g with cfirst[g] > c
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (cfirst[mid] <= c) lo = mid + 1;
    else hi = mid;
  }
  const int g = lo - 1, start = ftn_csr_offset(s, g) + (c - cfirst[g]) * FTN_GROUP_CHUNK;
  return FtnGroupChunk{g, start, ftn_csr_offset(s, g + 1) - start};
}

#ifdef __HIPCC__
// cfirst in LDS by the nthreads threads of a workgroup (part: nthreads words of LDS), ready for every thread on return
__device__ __forceinline__ void ftn_csr_first_wg(const FtnGroupCsr& s, int nthreads, int* part, int* cfirst) {
  int g0, g1;
  part[threadIdx.x] = ftn_csr_count(s, threadIdx.x, nthreads, &g0, &g1);
  __syncthreads();
  ftn_csr_first(s, threadIdx.x, nthreads, g0, g1, part, cfirst);
  __syncthreads();
}

// What both entries check about their pointers and the CSR before a launch; *chunks = the chunks of offsets_host.
static inline int group_csr_check(const char* who, const float* x_dev, const float* out_dev, const int* order_dev,
                                  const int* offsets_dev, const int* offsets_host, int G, int M, int* chunks) {
  FTN_CHECK_ARG(x_dev && out_dev && offsets_dev && offsets_host, "%s: null x, out or offsets", who);
  FTN_CHECK_ARG((((uintptr_t)x_dev | (uintptr_t)out_dev | (uintptr_t)order_dev | (uintptr_t)offsets_dev |
                  (uintptr_t)offsets_host) & 3) == 0, "%s: operands must be 4-byte aligned", who);
  FTN_CHECK_ARG(G >= 1 && G <= FTN_GROUP_GMAX, "%s: G=%d is outside 1..%d", who, G, FTN_GROUP_GMAX);
  FTN_CHECK_ARG(M >= 0 && (M == 0 || order_dev), "%s: M=%d members need order", who, M);
  FTN_CHECK_ARG(offsets_host[0] == 0 && offsets_host[G] == M, "%s: offsets run %d..%d, not 0..M=%d", who,
                offsets_host[0], offsets_host[G], M);
  long long n = 0;
  for (int g = 0; g < G; ++g) {
    const long long m = (long long)offsets_host[g + 1] - offsets_host[g];
    FTN_CHECK_ARG(m >= 0, "%s: offsets decrease at group %d", who, g);
    n += (m + FTN_GROUP_CHUNK - 1) / FTN_GROUP_CHUNK;
  }
  FTN_CHECK_ARG(n <= FTN_GROUP_CHUNKS_MAX, "%s: %lld chunks are above %d", who, n, FTN_GROUP_CHUNKS_MAX);
  *chunks = (int)n;
  return 0;
}
#endif
