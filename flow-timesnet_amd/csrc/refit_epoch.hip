// The end of a validated refit epoch, on the device (include/flowtimes.h, FtnEpochArgs; fit.EpochEnd): the
// reference's per-epoch bookkeeping - validation NLL and sMAPE from the scorer's accumulators, ReduceLROnPlateau,
// the best epoch, early stopping - decided and acted on without a host read, so that epochs can be enqueued back to
// back behind captured steps.
//   k_epoch_decide   one workgroup.  The accumulator records pass through LDS in tiles of EP_TILE: every thread
//                    stages records tid, tid + 256, ... and zeroes them in place (it is their only reader), then lane
//                    0 of wave 0 adds the tile's nll sums and counts and lane 0 of wave 1 its sMAPE sums and counts,
//                    each serially in slot order from 0.0 - the order of ForecastScorer.result().  Thread 0 then
//                    applies the rule and writes the state record, the optimiser's lr word and the log row.
//   k_epoch_copy     workgroup c copies chunk c of up to 8 tensors when its gate word says so (state.improved != 0
//                    after an epoch: parameters -> best-state store; state.best_epoch > 0 at the end: store ->
//                    parameters) and returns at once otherwise.  Units of 4 elements and chunks of units as
//                    ftn_refit_update deals them; 16-byte accesses where both addresses allow, scalars elsewhere.
// The gate is read from the record the decide kernel wrote in the launch before, on the same stream.  Plain vector
// stores, no atomics.  Kernels, the plan, the launches and the C entry points.
#include "ftn_common.h"

#include <math.h>

#define EP_THREADS 256
#define EP_TILE 1024                     // records staged per pass: 24 KB of LDS
#define EP_UNITS_PER_CHUNK 1024          // 4096 elements: four units a thread

struct EpochK {
  FtnScorePart* acc;
  int n_slots, max_epochs;
  const int* err;
  double* den_extra;
  long long* count_seen;
  FtnEpochState* state;
  float* lr;
  double* log;
  double factor, threshold, min_lr;
  int plateau_patience, patience_limit;
};

__global__ __launch_bounds__(EP_THREADS) void k_epoch_decide(EpochK a) {
#pragma clang fp contract(off)
  __shared__ double s_nll[EP_TILE], s_sm[EP_TILE];
  __shared__ int c_nll[EP_TILE], c_sm[EP_TILE];
  __shared__ double sm_total;
  __shared__ long long sm_count;
  const int tid = threadIdx.x;
  double sum = 0.0;
  long long count = 0;
  for (int t0 = 0; t0 < a.n_slots; t0 += EP_TILE) {
    const int m = a.n_slots - t0 < EP_TILE ? a.n_slots - t0 : EP_TILE;
    __syncthreads();                          // the tile before this one has been added up
    for (int i = tid; i < m; i += EP_THREADS) {
      FtnScorePart* r = a.acc + t0 + i;
      s_nll[i] = r->nll_sum;  s_sm[i] = r->smape_sum;
      c_nll[i] = r->nll_cnt;  c_sm[i] = r->smape_cnt;
      r->nll_sum = 0.0;  r->smape_sum = 0.0;  r->nll_cnt = 0;  r->smape_cnt = 0;
    }
    __syncthreads();
    if (tid == 0) {
      for (int i = 0; i < m; ++i) { sum += s_nll[i]; count += c_nll[i]; }
    } else if (tid == 64) {
      for (int i = 0; i < m; ++i) { sum += s_sm[i]; count += c_sm[i]; }
    }
  }
  if (tid == 64) { sm_total = sum; sm_count = count; }
  __syncthreads();
  if (tid != 0) return;

  const double den = (double)count + *a.den_extra;
  const double val_nll = den > 0.0 ? sum / den : 0.0;
  const double val_smape = sm_count > 0 ? sm_total / (double)sm_count : 0.0;
  *a.den_extra = 0.0;
  if (a.count_seen) *a.count_seen = 0;

  FtnEpochState s = *a.state;
  const bool plateau = a.plateau_patience >= 0;
  double* row = s.calls < a.max_epochs ? a.log + (size_t)s.calls * 5 : nullptr;
  s.calls += 1;
  if (s.stop != 0) {                          // 1. after the stop: the row and the call count alone
    if (row) {
      row[0] = __builtin_nan("");  row[1] = __builtin_nan("");
      row[2] = plateau ? s.lr : (double)*a.lr;  row[3] = (double)FTN_EPOCH_AFTER_STOP;  row[4] = 0.0;
    }
    a.state->calls = s.calls;
    return;
  }
  s.epoch += 1;                               // 2.
  const int flags = *a.err != 0 ? FTN_EPOCH_SCORER_ERR : 0;
  if (plateau) {                              // 3.
    if (val_nll < s.plateau_best * (1.0 - a.threshold)) {
      s.plateau_best = val_nll;
      s.num_bad = 0;
    } else {
      s.num_bad += 1;
    }
    if (s.num_bad > a.plateau_patience) {
      const double scaled = s.lr * a.factor;
      const double next = a.min_lr > scaled ? a.min_lr : scaled;
      if (s.lr - next > 1e-8) s.lr = next;
      s.num_bad = 0;
    }
    *a.lr = (float)s.lr;
  } else {
    s.lr = (double)*a.lr;
  }
  if (val_nll < s.best_nll) {                 // 4.
    s.best_nll = val_nll;  s.best_smape = val_smape;  s.best_epoch = s.epoch;  s.patience = 0;  s.improved = 1;
  } else {
    s.improved = 0;
    s.patience += 1;
    if (a.patience_limit >= 0 && s.patience > a.patience_limit) s.stop = FTN_EPOCH_STOP;
  }
  if (row) {                                  // 5.
    row[0] = val_nll;  row[1] = val_smape;  row[2] = s.lr;  row[3] = (double)flags;  row[4] = (double)s.improved;
  }
  *a.state = s;
}

struct EpochCopyK {
  const unsigned* src[FTN_EPOCH_MAX_TENSORS];
  unsigned* dst[FTN_EPOCH_MAX_TENSORS];
  unsigned n[FTN_EPOCH_MAX_TENSORS];            // elements
  unsigned ustart[FTN_EPOCH_MAX_TENSORS + 1];   // first unit of tensor i; [nt] = all units
  int nt, scalar_mask;
  unsigned chunk;
  const int* gate;
  int gate_positive;                            // 0: copy when *gate != 0; 1: copy when *gate > 0
};

typedef unsigned u4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(EP_THREADS) void k_epoch_copy(EpochCopyK a) {
  const int g = *a.gate;                        // uniform: one scalar load
  if (a.gate_positive ? g <= 0 : g == 0) return;
  const unsigned long long c0 = (unsigned long long)blockIdx.x * a.chunk, c1 = c0 + a.chunk;
#pragma unroll
  for (int i = 0; i < FTN_EPOCH_MAX_TENSORS; ++i) {
    if (i >= a.nt) break;
    const unsigned long long lo = c0 > a.ustart[i] ? c0 : a.ustart[i];
    const unsigned long long hi = c1 < a.ustart[i + 1] ? c1 : a.ustart[i + 1];
    const bool aligned = !(a.scalar_mask >> i & 1);
    for (unsigned long long u = lo + threadIdx.x; u < hi; u += EP_THREADS) {
      const unsigned e0 = (unsigned)(u - a.ustart[i]) * 4u;
      const unsigned left = a.n[i] - e0, cnt = left < 4u ? left : 4u;
      const unsigned* __restrict__ s = a.src[i] + e0;
      unsigned* __restrict__ d = a.dst[i] + e0;
      if (aligned && cnt == 4u) {
        *(u4*)d = *(const u4*)s;
      } else {
        for (unsigned k = 0; k < cnt; ++k) d[k] = s[k];
      }
    }
  }
}

// How the copy is dealt: the one place the choice is made - the launch dispatches on it and ftn_refit_epoch_form
// exports it.
struct EpochPlan {
  unsigned ustart[FTN_EPOCH_MAX_TENSORS + 1];
  unsigned chunk, chunks;
  int scalar_mask, form;
};

static bool ep_plan(int n, const long long* counts, const int* misalign_or, EpochPlan* pl) {
  if (n < 1 || n > FTN_EPOCH_MAX_TENSORS || !counts) return false;
  unsigned long long units = 0;
  pl->scalar_mask = 0;
  for (int i = 0; i < n; ++i) {
    if (counts[i] < 1 || counts[i] > 0x7fffffffLL) return false;
    if (misalign_or && !misalign_ok(misalign_or[i])) return false;
    if (misalign_or && misalign_or[i]) pl->scalar_mask |= 1 << i;
    pl->ustart[i] = (unsigned)units;
    units += ((unsigned long long)counts[i] + 3) / 4;
    if (units > 0x7fffffffULL) return false;
  }
  pl->ustart[n] = (unsigned)units;
  unsigned long long chunk = EP_UNITS_PER_CHUNK;
  if ((units + chunk - 1) / chunk > FTN_REFIT_PARTS_MAX) {
    chunk = (units + FTN_REFIT_PARTS_MAX - 1) / FTN_REFIT_PARTS_MAX;
    chunk = (chunk + EP_THREADS - 1) / EP_THREADS * EP_THREADS;
  }
  pl->chunk = (unsigned)chunk;
  pl->chunks = (unsigned)((units + chunk - 1) / chunk);
  pl->form = pl->scalar_mask ? FTN_EPOCH_COPY_MIXED : FTN_EPOCH_COPY_VEC;
  return true;
}

extern "C" int ftn_refit_epoch_form(int n, const long long* counts, const int* misalign_or) {
  EpochPlan pl;
  FTN_CHECK_ARG(ep_plan(n, counts, misalign_or, &pl),
                "ftn_refit_epoch_form: n=%d tensors (1..%d), every count >= 1, at most 2^31 - 1 units of 4 in all, "
                "misalign values on the 4-byte grid below 16", n, FTN_EPOCH_MAX_TENSORS);
  return pl.form | pl.scalar_mask << 4 | (int)pl.chunks << 12;
}

// Checks a tensor list and fills the copy's argument record and grid.
static int ep_copy_args(const char* who, int n, const float* const* src, float* const* dst, const long long* counts,
                        const int* gate, int gate_positive, EpochCopyK* k, unsigned* grid) {
  FTN_CHECK_ARG(n >= 1 && n <= FTN_EPOCH_MAX_TENSORS && src && dst && counts, "%s: %d tensors (1..%d)", who, n,
                FTN_EPOCH_MAX_TENSORS);
  int mis[FTN_EPOCH_MAX_TENSORS];
  for (int i = 0; i < n; ++i) {
    FTN_CHECK_ARG(counts[i] >= 1 && counts[i] <= 0x7fffffffLL, "%s: tensor %d has %lld elements (1 .. 2^31 - 1)", who,
                  i, counts[i]);
    FTN_CHECK_ARG(src[i] && dst[i], "%s: tensor %d has a null operand", who, i);
    const uintptr_t any = (uintptr_t)src[i] | (uintptr_t)dst[i];
    FTN_CHECK_ARG((any & 3) == 0, "%s: tensor %d has an operand off the 4-byte grid", who, i);
    FTN_CHECK_ARG(src[i] + counts[i] <= dst[i] || dst[i] + counts[i] <= src[i], "%s: tensor %d overlaps its copy", who,
                  i);
    mis[i] = (int)(any & 15);
  }
  EpochPlan pl;
  FTN_CHECK_ARG(ep_plan(n, counts, mis, &pl), "%s: more than 2^31 - 1 units of 4 elements", who);
  for (int i = 0; i < FTN_EPOCH_MAX_TENSORS; ++i) {
    const bool on = i < n;
    k->src[i] = on ? (const unsigned*)src[i] : nullptr;
    k->dst[i] = on ? (unsigned*)dst[i] : nullptr;
    k->n[i] = on ? (unsigned)counts[i] : 0u;
    k->ustart[i] = on ? pl.ustart[i] : pl.ustart[n];
  }
  k->ustart[FTN_EPOCH_MAX_TENSORS] = pl.ustart[n];
  k->nt = n; k->scalar_mask = pl.scalar_mask; k->chunk = pl.chunk; k->gate = gate; k->gate_positive = gate_positive;
  *grid = pl.chunks;
  return 0;
}

extern "C" int ftn_refit_epoch_end(const FtnEpochArgs* r, void* stream) {
  const char* who = "ftn_refit_epoch_end";
  FTN_CHECK_ARG(r != nullptr, "%s: null argument record", who);
  FTN_CHECK_ARG(r->acc_dev && r->n_slots >= 1 && ((uintptr_t)r->acc_dev & 7) == 0,
                "%s: %d accumulator records at an address that is null or off the 8-byte grid", who, r->n_slots);
  FTN_CHECK_ARG(r->max_epochs >= 1 && r->log_dev && ((uintptr_t)r->log_dev & 7) == 0,
                "%s: a log of %d rows (>= 1) at an address that is null or off the 8-byte grid", who, r->max_epochs);
  FTN_CHECK_ARG(r->err_dev && r->lr_dev && (((uintptr_t)r->err_dev | (uintptr_t)r->lr_dev) & 3) == 0,
                "%s: the error word and the lr word must be 4-byte aligned device words", who);
  FTN_CHECK_ARG(r->den_extra_dev && r->state_dev &&
                    (((uintptr_t)r->den_extra_dev | (uintptr_t)r->state_dev | (uintptr_t)r->count_seen_dev_or_null) & 7) == 0,
                "%s: den_extra, count_seen and the state record must be 8-byte aligned (the first and last not null)",
                who);
  if (r->plateau_patience >= 0)
    FTN_CHECK_ARG(r->factor > 0.0 && r->factor < 1.0 && r->threshold == r->threshold && r->min_lr >= 0.0,
                  "%s: plateau factor=%g (inside (0, 1)) threshold=%g min_lr=%g (>= 0)", who, r->factor, r->threshold,
                  r->min_lr);
  FTN_CHECK_ARG(r->n_tensors >= 0 && r->n_tensors <= FTN_EPOCH_MAX_TENSORS, "%s: %d tensors (0..%d)", who,
                r->n_tensors, FTN_EPOCH_MAX_TENSORS);
  EpochCopyK k;
  unsigned grid = 0;
  if (r->n_tensors > 0) {
    const int rc = ep_copy_args(who, r->n_tensors, r->src, r->dst, r->n, &r->state_dev->improved, 0, &k, &grid);
    if (rc != 0) return rc;
  }
  EpochK a;
  a.acc = r->acc_dev; a.n_slots = r->n_slots; a.max_epochs = r->max_epochs; a.err = r->err_dev;
  a.den_extra = r->den_extra_dev; a.count_seen = r->count_seen_dev_or_null; a.state = r->state_dev; a.lr = r->lr_dev;
  a.log = r->log_dev; a.factor = r->factor; a.threshold = r->threshold; a.min_lr = r->min_lr;
  a.plateau_patience = r->plateau_patience; a.patience_limit = r->patience_limit;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_epoch_decide, dim3(1), dim3(EP_THREADS), 0, st, a);
  FTN_CHECK_LAUNCH();
  if (r->n_tensors > 0) {
    hipLaunchKernelGGL(k_epoch_copy, dim3(grid), dim3(EP_THREADS), 0, st, k);
    FTN_CHECK_LAUNCH();
  }
  return 0;
}

extern "C" int ftn_refit_epoch_restore(const FtnEpochState* state_dev, int n_tensors, const float* const* src,
                                       float* const* dst, const long long* counts, void* stream) {
  const char* who = "ftn_refit_epoch_restore";
  FTN_CHECK_ARG(state_dev && ((uintptr_t)state_dev & 7) == 0, "%s: the state record is null or off the 8-byte grid", who);
  EpochCopyK k;
  unsigned grid = 0;
  const int rc = ep_copy_args(who, n_tensors, src, dst, counts, &state_dev->best_epoch, 1, &k, &grid);
  if (rc != 0) return rc;
  hipLaunchKernelGGL(k_epoch_copy, dim3(grid), dim3(EP_THREADS), 0, (hipStream_t)stream, k);
  FTN_CHECK_LAUNCH();
  return 0;
}
