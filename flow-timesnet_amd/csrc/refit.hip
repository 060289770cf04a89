// The optimiser step of a refit, on the device: clip by the global gradient norm, then AdamW, for up to
// FTN_REFIT_MAX_TENSORS fp32 tensors in one call (include/flowtimes.h, FtnRefitArgs).  Step count, learning rate,
// norm and the decision to skip the update are device words: nothing is read on the host, so the call can sit at the
// end of a captured training step.
//
// Work is dealt in units of 4 consecutive elements of one tensor (the last unit of a tensor holds n % 4 or 4); units
// of all tensors form one range, cut into chunks of `chunk` units.  A tensor whose four operands are on the 16-byte
// grid moves a full unit with one 16-byte access per operand and its tail unit with scalars; any other tensor moves
// every unit with scalars.  Either way a thread meets the same elements in the same order, so the form changes no bit.
//   sum of squares   thread: units lo + tid, lo + tid + 256, ... of each tensor's share of the chunk, tensors
//                    ascending, fp64, element by element; workgroup: xor butterfly over the wave, then the four wave
//                    sums ascending -> the chunk's partial; total: thread tid adds partials tid, tid + 256, ...
//                    ascending, then the same workgroup sum.  Every workgroup gets the same bits.
//   k_refit_one      one workgroup: every chunk's partial into LDS, the total, the decision, the update, the words
//   k_refit_norm     workgroup c: partial c into the workspace; workgroup 0 also copies t beside them
//   k_refit_apply    workgroup c: the total from the workspace, the decision, chunk c; workgroup 0 writes the words
// The apply kernel reads t from the workspace copy, not from state[], so the workgroup that advances t cannot be seen
// by a workgroup that starts later.  No atomics.  Kernels, the form rule, the launch and the C entry points.
// ftn_refit_update_list (at the end): one step over up to FTN_REFIT_LIST_MAX records - a k_refit_norm launch per
// record into one list of partials, then a k_refit_apply launch per record over the whole list.
#include "ftn_common.h"

#include <math.h>

#define RF_THREADS 256
#define RF_UNITS_PER_CHUNK 1024          // 4096 elements: four units a thread
#define RF_ONE_CHUNKS_CAP 64             // what k_refit_one's LDS holds (a forced form may go this far)
// k_refit_one up to this many chunks, the grid beyond.  Measured (profiles/refit_step_time.json, DESIGN section 4
// "Refit step"), eager calls of about 20 us of host time each: one launch is 2 us ahead of two at one and at two full
// chunks (20.3 against 22.1 us) and 4 us behind at four (26.4 against 22.3), where its one workgroup walks 16384
// elements; the lines cross between two and three full chunks.
#define RF_ONE_CHUNKS_MAX 2

struct RefitK {
  float* p[FTN_REFIT_MAX_TENSORS];
  const float* g[FTN_REFIT_MAX_TENSORS];
  float* m[FTN_REFIT_MAX_TENSORS];
  float* v[FTN_REFIT_MAX_TENSORS];
  unsigned n[FTN_REFIT_MAX_TENSORS];          // elements
  unsigned ustart[FTN_REFIT_MAX_TENSORS + 1]; // first unit of tensor i; [nt] = all units
  const int* skip[FTN_REFIT_MAX_SKIP];
  int nt, nskip, scalar_mask, range_mask;
  double beta1, beta2, eps, wd, max_norm;
  const float* lr;
  int* state;
  const float* loss;
  float* log;
  int cap;
  double* part;                               // [pall] partials, then one int: t as the norm kernel found it
  unsigned chunk, chunks;
  // ftn_refit_update_list: this record's partials are part[pbase .. pbase + chunks) of pall in all; the record that
  // copies t (the first) and the one that writes the words (the last).  One record: 0, chunks, both.
  unsigned pbase, pall;
  int copies_t, writes_words;
};

// What every thread of a call agrees on before it touches an element.
struct RefitStep {
  float c, decay, b1, omb1, b2, omb2, rs, eps, step, lr, loss;
  double norm;
  int flags;                                  // 0: update; else the log's flag bits
};

__device__ __forceinline__ double rf_block_sum(double v, double* wave_sums) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) v += __shfl_xor(v, off, 64);
  __syncthreads();                            // the previous use of wave_sums is over
  if ((threadIdx.x & 63) == 0) wave_sums[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((wave_sums[0] + wave_sums[1]) + wave_sums[2]) + wave_sums[3];
}

// Visits the units of chunk `c`: f(i, e0, cnt, vec) for tensor i, first element e0, cnt elements, vec: one 16-byte
// access per operand.  The tensor loop is unrolled so that no pointer of the argument record is indexed at run time.
template <typename F>
__device__ __forceinline__ void rf_walk(const RefitK& a, unsigned c, F&& f) {
  const unsigned long long c0 = (unsigned long long)c * a.chunk, c1 = c0 + a.chunk;
#pragma unroll
  for (int i = 0; i < FTN_REFIT_MAX_TENSORS; ++i) {
    if (i >= a.nt) break;
    const unsigned long long lo = c0 > a.ustart[i] ? c0 : a.ustart[i];
    const unsigned long long hi = c1 < a.ustart[i + 1] ? c1 : a.ustart[i + 1];
    const bool aligned = !(a.scalar_mask >> i & 1);
    for (unsigned long long u = lo + threadIdx.x; u < hi; u += RF_THREADS) {
      const unsigned e0 = (unsigned)(u - a.ustart[i]) * 4u;
      const unsigned left = a.n[i] - e0, cnt = left < 4u ? left : 4u;
      f(i, e0, cnt, aligned && cnt == 4u);
    }
  }
}

__device__ __forceinline__ double rf_chunk_squares(const RefitK& a, unsigned c) {
  double s = 0.0;
  rf_walk(a, c, [&](int i, unsigned e0, unsigned cnt, bool vec) {
    const float* __restrict__ g = a.g[i] + e0;
    if (vec) {
      const f4 x = *(const f4*)g;
#pragma unroll
      for (int k = 0; k < 4; ++k) s += (double)x[k] * (double)x[k];
    } else {
      for (unsigned k = 0; k < cnt; ++k) s += (double)g[k] * (double)g[k];
    }
  });
  return s;
}

// Partials tid, tid + 256, ... ascending, then the workgroup sum.
template <typename P>
__device__ __forceinline__ double rf_total(P part, unsigned chunks, double* wave_sums) {
  double s = 0.0;
  for (unsigned k = threadIdx.x; k < chunks; k += RF_THREADS) s += part[k];
  return rf_block_sum(s, wave_sums);
}

__device__ __forceinline__ double rf_powi(double b, int t) {     // b^t, t >= 1, by squaring
  double r = 1.0;
  while (t > 0) {
    if (t & 1) r *= b;
    b *= b;
    t >>= 1;
  }
  return r;
}

__device__ __forceinline__ RefitStep rf_decide(const RefitK& a, double total, int t) {
  RefitStep h;
  h.norm = sqrt(total);
  h.lr = *a.lr;
  h.loss = a.loss ? *a.loss : 0.f;
  int flags = 0;
#pragma unroll
  for (int k = 0; k < FTN_REFIT_MAX_SKIP; ++k) {
    if (k >= a.nskip) break;
    const int w = *a.skip[k];
    if (w != 0) flags |= (a.range_mask >> k & 1) ? 4 : (w & 3) | ((w & ~3) ? 8 : 0);   // a head's word: bits 0 and 1
  }
  if (!isfinite(h.norm) || !isfinite(h.loss)) flags |= 8;
  h.flags = flags;
  const double cd = a.max_norm > 0.0 ? a.max_norm / (h.norm + 1e-6) : 1.0;
  h.c = (float)(cd < 1.0 ? cd : 1.0);
  const int t1 = t + 1;
  const double bc1 = 1.0 - rf_powi(a.beta1, t1), bc2 = 1.0 - rf_powi(a.beta2, t1);
  h.decay = (float)(1.0 - (double)h.lr * a.wd);
  h.b1 = (float)a.beta1;  h.omb1 = (float)(1.0 - a.beta1);
  h.b2 = (float)a.beta2;  h.omb2 = (float)(1.0 - a.beta2);
  h.rs = (float)sqrt(bc2);
  h.eps = (float)a.eps;
  h.step = (float)((double)h.lr / bc1);
  return h;
}

// One element, every operation rounded once to fp32 and none fused but the two written as fmaf.
__device__ __forceinline__ void rf_adamw(float& p, float g, float& m, float& v, const RefitStep& h) {
#pragma clang fp contract(off)
  const float gc = h.c * g;
  const float pd = p * h.decay;
  m = __builtin_fmaf(h.b1, m, h.omb1 * gc);
  v = __builtin_fmaf(h.b2, v, (h.omb2 * gc) * gc);
  const float den = __builtin_sqrtf(v) / h.rs + h.eps;
  p = pd - h.step * (m / den);
}

__device__ __forceinline__ void rf_chunk_apply(const RefitK& a, unsigned c, const RefitStep& h) {
  rf_walk(a, c, [&](int i, unsigned e0, unsigned cnt, bool vec) {
    const float* __restrict__ g = a.g[i] + e0;
    float* p = a.p[i] + e0;
    float* m = a.m[i] + e0;
    float* v = a.v[i] + e0;
    if (vec) {
      const f4 gx = *(const f4*)g;
      f4 px = *(const f4*)p, mx = *(const f4*)m, vx = *(const f4*)v;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float pk = px[k], mk = mx[k], vk = vx[k];
        rf_adamw(pk, gx[k], mk, vk, h);
        px[k] = pk; mx[k] = mk; vx[k] = vk;
      }
      *(f4*)p = px; *(f4*)m = mx; *(f4*)v = vx;
    } else {
      for (unsigned k = 0; k < cnt; ++k) {
        float pk = p[k], mk = m[k], vk = v[k];
        rf_adamw(pk, g[k], mk, vk, h);
        p[k] = pk; m[k] = mk; v[k] = vk;
      }
    }
  });
}

// The call's words, by one thread: t advances with an update, calls always, the log row of this call.
__device__ __forceinline__ void rf_words(const RefitK& a, const RefitStep& h, int t) {
  const int calls = a.state[1];
  if (h.flags == 0) a.state[0] = t + 1;
  a.state[1] = calls + 1;
  if (a.cap > 0) {
    float* row = a.log + (size_t)(((unsigned)calls) % (unsigned)a.cap) * 4;
    row[0] = h.loss; row[1] = (float)h.norm; row[2] = h.lr; row[3] = (float)h.flags;
  }
}

__global__ __launch_bounds__(RF_THREADS) void k_refit_one(RefitK a) {
  __shared__ double wave_sums[4];
  __shared__ double part[RF_ONE_CHUNKS_CAP];
  const int t = a.state[0];
  for (unsigned c = 0; c < a.chunks; ++c) {
    const double s = rf_block_sum(rf_chunk_squares(a, c), wave_sums);
    if (threadIdx.x == 0) part[c] = s;
  }
  __syncthreads();
  const double total = rf_total((const double*)part, a.chunks, wave_sums);
  const RefitStep h = rf_decide(a, total, t);
  if (h.flags == 0)
    for (unsigned c = 0; c < a.chunks; ++c) rf_chunk_apply(a, c, h);
  __syncthreads();                            // every thread has read t
  if (threadIdx.x == 0) rf_words(a, h, t);
}

__global__ __launch_bounds__(RF_THREADS) void k_refit_norm(RefitK a) {
  __shared__ double wave_sums[4];
  const double s = rf_block_sum(rf_chunk_squares(a, blockIdx.x), wave_sums);
  if (threadIdx.x == 0) {
    a.part[a.pbase + blockIdx.x] = s;
    if (blockIdx.x == 0 && a.copies_t) *(int*)(a.part + a.pall) = a.state[0];
  }
}

__global__ __launch_bounds__(RF_THREADS) void k_refit_apply(RefitK a) {
  __shared__ double wave_sums[4];
  const int t = *(const int*)(a.part + a.pall);
  const double total = rf_total((const double*)a.part, a.pall, wave_sums);
  const RefitStep h = rf_decide(a, total, t);
  if (h.flags == 0) rf_chunk_apply(a, blockIdx.x, h);
  if (blockIdx.x == 0 && threadIdx.x == 0 && a.writes_words) rf_words(a, h, t);
}

// The form ftn_refit_update takes (include/flowtimes.h): the one place the choice is made - the launch below
// dispatches on this value and ftn_refit_update_form exports it.
struct RefitPlan {
  unsigned ustart[FTN_REFIT_MAX_TENSORS + 1];
  unsigned chunk, chunks;
  int scalar_mask, form;
};

static bool rf_plan(int n, const long long* counts, const int* misalign_or, RefitPlan* pl) {
  if (n < 1 || n > FTN_REFIT_MAX_TENSORS || !counts) return false;
  unsigned long long units = 0;
  pl->scalar_mask = 0;
  for (int i = 0; i < n; ++i) {
    if (counts[i] < 1 || counts[i] > 0x7fffffffLL) return false;
    if (misalign_or && (misalign_or[i] < 0 || misalign_or[i] > 15 || misalign_or[i] % 4)) return false;
    if (misalign_or && misalign_or[i]) pl->scalar_mask |= 1 << i;
    pl->ustart[i] = (unsigned)units;
    units += ((unsigned long long)counts[i] + 3) / 4;
    if (units > 0x7fffffffULL) return false;
  }
  pl->ustart[n] = (unsigned)units;
  unsigned long long chunk = RF_UNITS_PER_CHUNK;
  if ((units + chunk - 1) / chunk > FTN_REFIT_PARTS_MAX) {
    chunk = (units + FTN_REFIT_PARTS_MAX - 1) / FTN_REFIT_PARTS_MAX;
    chunk = (chunk + RF_THREADS - 1) / RF_THREADS * RF_THREADS;
  }
  pl->chunk = (unsigned)chunk;
  pl->chunks = (unsigned)((units + chunk - 1) / chunk);
  pl->form = pl->chunks <= RF_ONE_CHUNKS_MAX ? FTN_REFIT_ONE : FTN_REFIT_GRID;
  return true;
}

extern "C" int ftn_refit_update_form(int n, const long long* counts, const int* misalign_or) {
  RefitPlan pl;
  FTN_CHECK_ARG(rf_plan(n, counts, misalign_or, &pl),
                "ftn_refit_update_form: n=%d tensors (1..%d), every count >= 1, at most 2^31 - 1 units of 4 in all, "
                "misalign values on the 4-byte grid below 16", n, FTN_REFIT_MAX_TENSORS);
  return pl.form | pl.scalar_mask << 4 | (int)pl.chunks << 12;
}

extern "C" size_t ftn_refit_update_workspace(int n, const long long* counts) {
  RefitPlan pl;
  if (!rf_plan(n, counts, nullptr, &pl)) return 0;
  return (size_t)pl.chunks * sizeof(double) + 16;
}

// One record's checks and its kernel arguments: everything but the workspace, which the two entries lay out.
static int rf_record(const char* who, const FtnRefitArgs* r, RefitPlan& pl, RefitK& a) {
  FTN_CHECK_ARG(r != nullptr, "%s: null argument record", who);
  FTN_CHECK_ARG(r->n_tensors >= 1 && r->n_tensors <= FTN_REFIT_MAX_TENSORS, "%s: %d tensors (1..%d)", who, r->n_tensors,
                FTN_REFIT_MAX_TENSORS);
  int mis[FTN_REFIT_MAX_TENSORS];
  for (int i = 0; i < r->n_tensors; ++i) {
    FTN_CHECK_ARG(r->n[i] >= 1, "%s: tensor %d has %lld elements (>= 1)", who, i, r->n[i]);
    FTN_CHECK_ARG(r->p[i] && r->g[i] && r->m[i] && r->v[i], "%s: tensor %d has a null operand", who, i);
    const uintptr_t any = (uintptr_t)r->p[i] | (uintptr_t)r->g[i] | (uintptr_t)r->m[i] | (uintptr_t)r->v[i];
    FTN_CHECK_ARG((any & 3) == 0, "%s: tensor %d has an operand off the 4-byte grid", who, i);
    mis[i] = (int)(any & 15);
  }
  FTN_CHECK_ARG(rf_plan(r->n_tensors, r->n, mis, &pl), "%s: more than 2^31 - 1 units of 4 elements", who);
  FTN_CHECK_ARG(r->lr_dev && r->state_dev && ((uintptr_t)r->lr_dev & 3) == 0 && ((uintptr_t)r->state_dev & 3) == 0,
                "%s: the lr word and state[2] must be 4-byte aligned device words", who);
  FTN_CHECK_ARG(r->beta1 >= 0.0 && r->beta1 < 1.0 && r->beta2 >= 0.0 && r->beta2 < 1.0 && r->eps >= 0.0 &&
                    r->weight_decay >= 0.0 && r->max_norm == r->max_norm,
                "%s: beta1=%g beta2=%g (in [0, 1)) eps=%g weight_decay=%g (>= 0) max_norm=%g", who, r->beta1, r->beta2,
                r->eps, r->weight_decay, r->max_norm);
  FTN_CHECK_ARG(r->n_skip >= 0 && r->n_skip <= FTN_REFIT_MAX_SKIP && (r->range_mask >> r->n_skip) == 0 && r->range_mask >= 0,
                "%s: %d skip words (0..%d), range_mask=%d", who, r->n_skip, FTN_REFIT_MAX_SKIP, r->range_mask);
  for (int k = 0; k < r->n_skip; ++k)
    FTN_CHECK_ARG(r->skip_dev[k] && ((uintptr_t)r->skip_dev[k] & 3) == 0, "%s: skip word %d is null or misaligned", who, k);
  FTN_CHECK_ARG(((uintptr_t)r->loss_dev_or_null & 3) == 0, "%s: the loss word must be 4-byte aligned", who);
  FTN_CHECK_ARG(r->log_cap >= 0 && (r->log_cap == 0) == (r->log_dev_or_null == nullptr) &&
                    ((uintptr_t)r->log_dev_or_null & 3) == 0,
                "%s: log of %d rows with %s buffer", who, r->log_cap, r->log_dev_or_null ? "a" : "no");
  for (int i = 0; i < FTN_REFIT_MAX_TENSORS; ++i) {
    const bool on = i < r->n_tensors;
    a.p[i] = on ? r->p[i] : nullptr;  a.g[i] = on ? r->g[i] : nullptr;
    a.m[i] = on ? r->m[i] : nullptr;  a.v[i] = on ? r->v[i] : nullptr;
    a.n[i] = on ? (unsigned)r->n[i] : 0u;
    a.ustart[i] = on ? pl.ustart[i] : pl.ustart[r->n_tensors];
  }
  a.ustart[FTN_REFIT_MAX_TENSORS] = pl.ustart[r->n_tensors];
  for (int k = 0; k < FTN_REFIT_MAX_SKIP; ++k) a.skip[k] = k < r->n_skip ? r->skip_dev[k] : nullptr;
  a.nt = r->n_tensors; a.nskip = r->n_skip; a.scalar_mask = pl.scalar_mask; a.range_mask = r->range_mask;
  a.beta1 = r->beta1; a.beta2 = r->beta2; a.eps = r->eps; a.wd = r->weight_decay; a.max_norm = r->max_norm;
  a.lr = r->lr_dev; a.state = r->state_dev; a.loss = r->loss_dev_or_null; a.log = r->log_dev_or_null; a.cap = r->log_cap;
  a.part = nullptr; a.chunk = pl.chunk; a.chunks = pl.chunks;
  a.pbase = 0; a.pall = pl.chunks; a.copies_t = 1; a.writes_words = 1;
  return 0;
}

extern "C" int ftn_refit_update(const FtnRefitArgs* r, void* stream) {
  const char* who = "ftn_refit_update";
  RefitPlan pl;
  RefitK a;
  if (int rc = rf_record(who, r, pl, a)) return rc;
  int form = pl.form;
  if (r->force_form != 0) {
    FTN_CHECK_ARG(r->force_form == FTN_REFIT_GRID || (r->force_form == FTN_REFIT_ONE && pl.chunks <= RF_ONE_CHUNKS_CAP),
                  "%s: force_form=%d with %u chunks (FTN_REFIT_ONE up to %d chunks, or FTN_REFIT_GRID)", who,
                  r->force_form, pl.chunks, RF_ONE_CHUNKS_CAP);
    form = r->force_form;
  }
  const size_t need = (size_t)pl.chunks * sizeof(double) + 16;
  if (form == FTN_REFIT_GRID)
    FTN_CHECK_ARG(r->workspace_dev && ((uintptr_t)r->workspace_dev & 7) == 0 && r->workspace_bytes >= need,
                  "%s: workspace of %zu bytes, %zu needed on the 8-byte grid (ftn_refit_update_workspace)", who,
                  r->workspace_bytes, need);
  a.part = (double*)r->workspace_dev;
  hipStream_t st = (hipStream_t)stream;
  if (form == FTN_REFIT_ONE) {
    hipLaunchKernelGGL(k_refit_one, dim3(1), dim3(RF_THREADS), 0, st, a);
    FTN_CHECK_LAUNCH();
    return 0;
  }
  hipLaunchKernelGGL(k_refit_norm, dim3(pl.chunks), dim3(RF_THREADS), 0, st, a);
  FTN_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_refit_apply, dim3(pl.chunks), dim3(RF_THREADS), 0, st, a);
  FTN_CHECK_LAUNCH();
  return 0;
}

// ---------------------------------------------------------------------------------------------
// One step over a list of records (include/flowtimes.h, ftn_refit_update_list)
// ---------------------------------------------------------------------------------------------
extern "C" size_t ftn_refit_update_list_workspace(int n_calls, const int* n_tensors, const long long* const* counts) {
  if (n_calls < 1 || n_calls > FTN_REFIT_LIST_MAX || !n_tensors || !counts) return 0;
  size_t chunks = 0;
  for (int c = 0; c < n_calls; ++c) {
    RefitPlan pl;
    if (!rf_plan(n_tensors[c], counts[c], nullptr, &pl)) return 0;
    chunks += pl.chunks;
  }
  return chunks * sizeof(double) + 16;
}

extern "C" int ftn_refit_update_list(const FtnRefitArgs* calls, int n_calls, void* workspace_dev,
                                     size_t workspace_bytes, void* stream) {
  const char* who = "ftn_refit_update_list";
  FTN_CHECK_ARG(calls != nullptr && n_calls >= 1 && n_calls <= FTN_REFIT_LIST_MAX, "%s: %d records (1..%d)", who, n_calls,
                FTN_REFIT_LIST_MAX);
  if (n_calls == 1) {                         // ftn_refit_update itself, on this workspace
    FtnRefitArgs one = calls[0];
    one.workspace_dev = workspace_dev;
    one.workspace_bytes = workspace_bytes;
    one.force_form = 0;
    return ftn_refit_update(&one, stream);
  }
  RefitPlan pl[FTN_REFIT_LIST_MAX];
  RefitK a[FTN_REFIT_LIST_MAX];
  unsigned pall = 0;
  const FtnRefitArgs& f = calls[0];
  for (int c = 0; c < n_calls; ++c) {
    const FtnRefitArgs& r = calls[c];
    if (int rc = rf_record(who, &r, pl[c], a[c])) return rc;
    bool same = r.beta1 == f.beta1 && r.beta2 == f.beta2 && r.eps == f.eps && r.weight_decay == f.weight_decay &&
                r.max_norm == f.max_norm && r.lr_dev == f.lr_dev && r.state_dev == f.state_dev && r.n_skip == f.n_skip &&
                r.range_mask == f.range_mask && r.log_cap == f.log_cap && r.loss_dev_or_null == f.loss_dev_or_null &&
                r.log_dev_or_null == f.log_dev_or_null;
    for (int k = 0; same && k < f.n_skip; ++k) same = r.skip_dev[k] == f.skip_dev[k];
    FTN_CHECK_ARG(same, "%s: record %d differs from record 0 in a hyper-parameter or a device word", who, c);
    a[c].pbase = pall;
    pall += pl[c].chunks;
  }
  const size_t need = (size_t)pall * sizeof(double) + 16;
  FTN_CHECK_ARG(workspace_dev && ((uintptr_t)workspace_dev & 7) == 0 && workspace_bytes >= need,
                "%s: workspace of %zu bytes, %zu needed on the 8-byte grid (ftn_refit_update_list_workspace)", who,
                workspace_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  for (int c = 0; c < n_calls; ++c) {
    a[c].part = (double*)workspace_dev;
    a[c].pall = pall;
    a[c].copies_t = c == 0;
    a[c].writes_words = c == n_calls - 1;
    hipLaunchKernelGGL(k_refit_norm, dim3(pl[c].chunks), dim3(RF_THREADS), 0, st, a[c]);
    FTN_CHECK_LAUNCH();
  }
  for (int c = 0; c < n_calls; ++c) {
    hipLaunchKernelGGL(k_refit_apply, dim3(pl[c].chunks), dim3(RF_THREADS), 0, st, a[c]);
    FTN_CHECK_LAUNCH();
  }
  return 0;
}
