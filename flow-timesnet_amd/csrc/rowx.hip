// Row exchange of a series-sharded forward (include/flowtimes.h, FtnRowExchange, ABI 13):
//   k_rowx_push    copy this rank's rows into slot `rank` of every destination's buffer, then turn one sequence word
//                  per (source, chunk) - the k_colsum pattern, one chunk of FTN_ROWX_CHUNK floats per workgroup
//   k_rowx_reduce  bounded wait for the words of the chunks a tile needs, sum the W slots in rank order, + add,
//                  optional LayerNorm over D -> out[R][L][D]
//   k_rowx_gather  bounded wait per chunk, copy the W slots -> out[W*R][width]
// The consumers are grid-stride loops over a bounded grid (ROWX_MAX_WG): a waiting workgroup holds its CU slot, and a
// peer that shares the GPU (two ranks on one device) must still find room for its push.
#include <string.h>
#include "ftn_common.h"
#include "ftn_exchange.h"

#define ROWX_MAX_WG 1024
#define ROWX_TIMEOUT_TICKS 200000000ull       // s_memrealtime ticks at 100 MHz: 2 s, as the [F] exchange

static inline size_t rowx_align(size_t v) { return (v + 255) & ~(size_t)255; }

// one half: [W][R*width] floats, then (256-byte aligned) [W][nblk] sequence words
struct RowxGeom {
  size_t slot_floats, flags_off, half_bytes;
  int nblk;
};
static bool rowx_geom(int world, int rows, int width, RowxGeom* g) {
  if (world < 1 || world > FTN_XCHG_MAXWORLD || rows < 1 || width < 4 || width % 4 != 0) return false;
  const size_t sf = (size_t)rows * (size_t)width;
  if (sf > ((size_t)1 << 28)) return false;
  g->slot_floats = sf;
  g->nblk = (int)((sf + FTN_ROWX_CHUNK - 1) / FTN_ROWX_CHUNK);
  g->flags_off = rowx_align((size_t)world * sf * sizeof(float));
  g->half_bytes = g->flags_off + rowx_align((size_t)world * g->nblk * 8);
  return true;
}
static size_t rowx_tail_off(const RowxGeom& g) { return 2 * g.half_bytes; }

struct RowxArgs {
  char* base[FTN_XCHG_MAXWORLD];      // every rank's buffer (half 0)
  size_t slot_floats, flags_off, half_bytes;
  int nblk, world, rank;
  unsigned long long* ctr;            // this rank's call counter
  unsigned int* ticket;               // this rank's workgroup ticket (consumers)
  int* err;                           // this rank's error word
};

static bool rowx_args(const FtnRowExchange* x, RowxArgs* a) {
  RowxGeom g;
  if (!x || !rowx_geom(x->world, x->rows_per_rank, x->width, &g) || x->rank < 0 || x->rank >= x->world ||
      (x->kind != 0 && x->kind != 1))
    return false;
  for (int r = 0; r < x->world; ++r)
    if (x->slots[r] == nullptr) return false;
  memset(a, 0, sizeof(*a));
  for (int r = 0; r < x->world; ++r) a->base[r] = (char*)x->slots[r];
  a->slot_floats = g.slot_floats; a->flags_off = g.flags_off; a->half_bytes = g.half_bytes;
  a->nblk = g.nblk; a->world = x->world; a->rank = x->rank;
  char* tail = (char*)x->slots[x->rank] + rowx_tail_off(g);
  a->err = (int*)tail;
  a->ctr = (unsigned long long*)(tail + 8);
  a->ticket = (unsigned int*)(tail + 16);
  return true;
}

// the counter is read and written only by the GPU that owns the buffer, in stream order: agent scope
__device__ __forceinline__ unsigned long long rowx_seq(const unsigned long long* ctr) {
  return __hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1;
}

// Wait until the words [s][b0..b1] of every source s have turned seq (or the budget ran out): the workgroup's threads
// poll one word each; returns nonzero (for every thread) when a word was late.  System-scope loads and an acquire
// fence: the words and the slots behind them were written by other GPUs or processes.
__device__ bool rowx_wait(const unsigned long long* flags, int nblk, int world, int b0, int b1, unsigned long long seq,
                          bool late, int* sh_late) {
  const int tid = threadIdx.x, per = b1 - b0 + 1;
  if (tid == 0) *sh_late = late ? 1 : 0;
  __syncthreads();
  if (!late) {
    for (int i = tid; i < world * per; i += blockDim.x) {
      const unsigned long long* w = flags + (size_t)(i / per) * nblk + b0 + i % per;
      const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
      while (__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != seq) {
        if (__builtin_amdgcn_s_memrealtime() - t0 > ROWX_TIMEOUT_TICKS) { *sh_late = 1; break; }
        __builtin_amdgcn_s_sleep(8);
      }
    }
  }
  __threadfence_system();
  __syncthreads();
  return *sh_late != 0;
}

// the last consumer workgroup to finish stores counter = seq: every workgroup has read its slots by then
__device__ void rowx_done(const RowxArgs& a, unsigned long long seq, bool late) {
  __syncthreads();
  if (threadIdx.x != 0) return;
  if (late) __hip_atomic_store(a.err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  const unsigned int t = __hip_atomic_fetch_add(a.ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
  if (t == gridDim.x - 1) {
    __hip_atomic_store(a.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(a.ctr, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// grid (nblk, world): workgroup (b, q) copies chunk b of the rows bound for rank q (row block q for a reduce-scatter,
// the same rows for every q in an all-gather) into slot `rank` of q's buffer, then releases and turns word [rank][b]
__global__ __launch_bounds__(256) void k_rowx_push(const float* __restrict__ src, RowxArgs a, int scatter) {
  const unsigned long long seq = rowx_seq(a.ctr);
  const int b = blockIdx.x, q = blockIdx.y;
  const size_t hoff = (size_t)(seq & 1) * a.half_bytes;
  const f4* s4 = (const f4*)(src + (scatter ? (size_t)q * a.slot_floats : 0));
  f4* d4 = (f4*)((float*)(a.base[q] + hoff) + (size_t)a.rank * a.slot_floats);
  const size_t i0 = (size_t)b * (FTN_ROWX_CHUNK / 4);
  size_t i1 = i0 + FTN_ROWX_CHUNK / 4;
  if (i1 > a.slot_floats / 4) i1 = a.slot_floats / 4;
  for (size_t i = i0 + threadIdx.x; i < i1; i += 256) d4[i] = s4[i];
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0)
    __hip_atomic_store((unsigned long long*)(a.base[q] + hoff + a.flags_off) + (size_t)a.rank * a.nblk + b, seq,
                       __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// LPR lanes per [D] row (D/4 rounded up to a power of two, <= 32): one float4 per lane; 256 / LPR rows per tile
template <int LPR>
__global__ __launch_bounds__(256) void k_rowx_reduce(RowxArgs a, int nrow, int D, const float* __restrict__ add,
                                                     long long add_bs, int L, const float* __restrict__ g,
                                                     const float* __restrict__ be, float eps, float* __restrict__ out) {
  constexpr int RPT = 256 / LPR;
  __shared__ int sh_late;
  const unsigned long long seq = rowx_seq(a.ctr);
  const size_t hoff = (size_t)(seq & 1) * a.half_bytes;
  const char* mine = a.base[a.rank] + hoff;
  const float* slots = (const float*)mine;
  const unsigned long long* flags = (const unsigned long long*)(mine + a.flags_off);
  const int sub = threadIdx.x % LPR, ri = threadIdx.x / LPR;
  const int c = 4 * sub;
  const float invD = 1.f / (float)D;
  const int ntile = (nrow + RPT - 1) / RPT;
  bool late = false;
  for (int t = blockIdx.x; t < ntile; t += gridDim.x) {
    const int r0 = t * RPT, r1 = min(r0 + RPT, nrow);
    late = rowx_wait(flags, a.nblk, a.world, (int)((size_t)r0 * D / FTN_ROWX_CHUNK),
                     (int)(((size_t)r1 * D - 1) / FTN_ROWX_CHUNK), seq, late, &sh_late);
    const int row = r0 + ri;
    const bool on = row < nrow && c < D;
    f4 v = {0.f, 0.f, 0.f, 0.f};
    if (on) {
      const size_t off = (size_t)row * D + c;
      v = *(const f4*)(slots + off);
      for (int s = 1; s < a.world; ++s) v += *(const f4*)(slots + (size_t)s * a.slot_floats + off);
      if (add) v += *(const f4*)(add + (size_t)(row / L) * add_bs + (size_t)(row % L) * D + c);
    }
    if (g) {
      float s = on ? v[0] + v[1] + v[2] + v[3] : 0.f;
#pragma unroll
      for (int m = LPR / 2; m > 0; m >>= 1) s += __shfl_xor(s, m, LPR);
      const float mean = s * invD;
      const f4 dv = v - mean;
      float q = on ? dv[0] * dv[0] + dv[1] * dv[1] + dv[2] * dv[2] + dv[3] * dv[3] : 0.f;
#pragma unroll
      for (int m = LPR / 2; m > 0; m >>= 1) q += __shfl_xor(q, m, LPR);
      const float rstd = rsqrtf(q * invD + eps);
      if (on) v = dv * rstd * *(const f4*)(g + c) + *(const f4*)(be + c);
    }
    if (late) v = f4{NAN, NAN, NAN, NAN};
    if (on) *(f4*)(out + (size_t)row * D + c) = v;
  }
  rowx_done(a, seq, late);
}

// one work item = (source s, chunk b): wait for word [s][b], copy the chunk of slot s to out row block s
__global__ __launch_bounds__(256) void k_rowx_gather(RowxArgs a, float* __restrict__ out) {
  __shared__ int sh_late;
  const unsigned long long seq = rowx_seq(a.ctr);
  const size_t hoff = (size_t)(seq & 1) * a.half_bytes;
  const char* mine = a.base[a.rank] + hoff;
  const unsigned long long* flags = (const unsigned long long*)(mine + a.flags_off);
  const int nitem = a.world * a.nblk;
  bool late = false;
  for (int it = blockIdx.x; it < nitem; it += gridDim.x) {
    const int s = it / a.nblk, b = it % a.nblk;
    // one source per item: the wait covers words [s][b] only
    late = rowx_wait(flags + (size_t)s * a.nblk, a.nblk, 1, b, b, seq, late, &sh_late);
    const f4* s4 = (const f4*)((const float*)mine + (size_t)s * a.slot_floats);
    f4* d4 = (f4*)(out + (size_t)s * a.slot_floats);
    const size_t i0 = (size_t)b * (FTN_ROWX_CHUNK / 4);
    size_t i1 = i0 + FTN_ROWX_CHUNK / 4;
    if (i1 > a.slot_floats / 4) i1 = a.slot_floats / 4;
    for (size_t i = i0 + threadIdx.x; i < i1; i += 256) d4[i] = late ? f4{NAN, NAN, NAN, NAN} : s4[i];
  }
  rowx_done(a, seq, late);
}

// ---- host side -------------------------------------------------------------------------------------------------
extern "C" size_t ftn_rowx_bytes(int world, int rows_per_rank, int width) {
  RowxGeom g;
  if (!rowx_geom(world, rows_per_rank, width, &g)) return 0;
  return rowx_tail_off(g) + 256;
}

// No plain-hipMalloc fallback: a cached buffer could serve a peer's rows from a stale L2 line.
extern "C" int ftn_rowx_alloc(int world, int rows_per_rank, int width, void** buf_out, void* handle64_out) {
  const size_t n = ftn_rowx_bytes(world, rows_per_rank, width);
  FTN_CHECK_ARG(n > 0 && buf_out && handle64_out, "ftn_rowx_alloc: world=%d rows_per_rank=%d width=%d", world,
                rows_per_rank, width);
  return ftn_ipc_alloc(n, false, "ftn_rowx_alloc", buf_out, handle64_out);
}
extern "C" int ftn_rowx_open(const void* handle64, void** mapped_out) {
  return ftn_ipc_open("ftn_rowx_open", "ftn_rowx_open", handle64, mapped_out);
}
extern "C" int ftn_rowx_close(void* mapped) { return ftn_ipc_close("ftn_rowx_close", mapped); }
extern "C" int ftn_rowx_free(void* buf) { return ftn_ipc_free("ftn_rowx_free", buf); }

static int rowx_read(const void* dev, void* host, size_t n, void* stream, const char* what) {
  hipError_t e = hipMemcpyAsync(host, dev, n, hipMemcpyDeviceToHost, (hipStream_t)stream);
  if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
  if (e != hipSuccess) { ftn_set_error("%s: %s", what, hipGetErrorString(e)); return (int)e; }
  return 0;
}
extern "C" int ftn_rowx_error(const FtnRowExchange* xch, void* stream) {
  RowxArgs a;
  FTN_CHECK_ARG(rowx_args(xch, &a), "ftn_rowx_error: bad row exchange");
  int v = 0;
  const int rc = rowx_read(a.err, &v, sizeof(v), stream, "ftn_rowx_error");
  return rc != 0 ? -rc - 1000 : v;
}
extern "C" int64_t ftn_rowx_calls(const FtnRowExchange* xch, void* stream) {
  RowxArgs a;
  FTN_CHECK_ARG(rowx_args(xch, &a), "ftn_rowx_calls: bad row exchange");
  unsigned long long v = 0;
  return rowx_read(a.ctr, &v, sizeof(v), stream, "ftn_rowx_calls") != 0 ? -1 : (int64_t)v;
}

extern "C" int ftn_rowx_push(const float* src_dev, const FtnRowExchange* xch, void* stream) {
  RowxArgs a;
  FTN_CHECK_ARG(src_dev && ((uintptr_t)src_dev & 15) == 0, "ftn_rowx_push: src must be a 16-byte aligned pointer");
  FTN_CHECK_ARG(rowx_args(xch, &a), "ftn_rowx_push: bad row exchange (world / rank / rows / width / kind / slots)");
  hipLaunchKernelGGL(k_rowx_push, dim3(a.nblk, a.world), dim3(256), 0, (hipStream_t)stream, src_dev, a,
                     xch->kind == 0 ? 1 : 0);
  FTN_CHECK_LAUNCH();
  return 0;
}

extern "C" int ftn_rowx_reduce(const FtnRowExchange* xch, int L, int D, const float* add_dev_or_null,
                               long long add_bstride, const float* ln_gamma_dev_or_null,
                               const float* ln_beta_dev_or_null, float ln_eps, float* out_dev, void* stream) {
  RowxArgs a;
  FTN_CHECK_ARG(out_dev, "ftn_rowx_reduce: null pointer");
  FTN_CHECK_ARG(rowx_args(xch, &a) && xch->kind == 0, "ftn_rowx_reduce: bad row exchange (or not kind 0)");
  FTN_CHECK_ARG(D >= 4 && D % 4 == 0 && D <= 128 && L >= 1 && (long long)L * D == xch->width,
                "ftn_rowx_reduce: L=%d D=%d do not match width=%d (D a multiple of 4, <= 128)", L, D, xch->width);
  FTN_CHECK_ARG((ln_gamma_dev_or_null == nullptr) == (ln_beta_dev_or_null == nullptr),
                "ftn_rowx_reduce: LayerNorm needs both gamma and beta");
  FTN_CHECK_ARG(add_bstride == 0 || add_bstride == (long long)L * D, "ftn_rowx_reduce: add_bstride must be 0 or L*D");
  FTN_CHECK_ARG((((uintptr_t)out_dev | (uintptr_t)add_dev_or_null | (uintptr_t)ln_gamma_dev_or_null |
                  (uintptr_t)ln_beta_dev_or_null) & 15) == 0,
                "ftn_rowx_reduce: out / add / LayerNorm parameters must be 16-byte aligned");
  const int nrow = xch->rows_per_rank * L;
  hipStream_t st = (hipStream_t)stream;
  auto go = [&](auto kern, int rpt) {
    const int grid = min(ftn_cdiv(nrow, rpt), ROWX_MAX_WG);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, st, a, nrow, D, add_dev_or_null, add_bstride, L,
                       ln_gamma_dev_or_null, ln_beta_dev_or_null, ln_eps, out_dev);
  };
  if (D <= 16) go(k_rowx_reduce<4>, 64);
  else if (D <= 32) go(k_rowx_reduce<8>, 32);
  else if (D <= 64) go(k_rowx_reduce<16>, 16);
  else go(k_rowx_reduce<32>, 8);
  FTN_CHECK_LAUNCH();
  return 0;
}

extern "C" int ftn_rowx_gather(const FtnRowExchange* xch, float* out_dev, void* stream) {
  RowxArgs a;
  FTN_CHECK_ARG(out_dev && ((uintptr_t)out_dev & 15) == 0, "ftn_rowx_gather: out must be a 16-byte aligned pointer");
  FTN_CHECK_ARG(rowx_args(xch, &a) && xch->kind == 1, "ftn_rowx_gather: bad row exchange (or not kind 1)");
  const int grid = min(a.world * a.nblk, ROWX_MAX_WG);
  hipLaunchKernelGGL(k_rowx_gather, dim3(grid), dim3(256), 0, (hipStream_t)stream, a, out_dev);
  FTN_CHECK_LAUNCH();
  return 0;
}
