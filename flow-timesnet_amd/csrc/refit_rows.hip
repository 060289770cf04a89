// The rest of a cached refit batch in one launch (fit.OutputCache / fit.GraphedCachedStep): what the head kernels and
// the loss read as contiguous batch tensors, formed from the per-item stores through the step's row list.
//   tail [n_items][hist N] -> [B][hist N]        y, mask, late [n_items][S N] -> [B][S N]     (mask, late optional)
// seq is not copied: the time projection's two kernels read its store in place through the same list (the _rows
// entries of timeproj.hip and timeproj_bwd.hip).  Every operand here is S N floats an item or fewer, so this is row
// copies on the VALU: workgroup b moves item store_row(rows, n_items, b) into batch row b, a row with 16-byte
// accesses when its length is a multiple of 4 floats and both of its bases are on the 16-byte grid, else float by
// float.  Two more things ride along:
//   rows_ok [B]   the clamped list, which the step hands to the _rows entries
//   status        one int32: FTN_REFIT_ROWS_BAD when any rows[b] was outside 0 .. n_items - 1, else 0.  Workgroup 0
//                 alone reads the whole list for it (8 B bytes, from L2) and its thread 0 stores the word, so no
//                 workgroup waits for another, there is no atomic, and every call rewrites the word.
// The word is a skip word of ftn_refit_update: a step with a bad index leaves parameters and moments as they were.
// The kernel, the launch and the C entry point.
#include "ftn_common.h"

#define RR_THREADS 256

struct RefitRowsArgs {
  const long long* rows;     // [B]
  long long n_items;
  const float* src[4];       // tail, y, mask, late stores (null: absent)
  float* dst[4];
  int floats[4];             // floats of an item's row
  int vec;                   // bit k: operand k moves with 16-byte accesses
  long long* rows_ok;        // [B]
  int* status;
  int B;
};

__global__ __launch_bounds__(RR_THREADS) void k_refit_rows_gather(RefitRowsArgs a) {
  const int b = blockIdx.x;
  const long long r = store_row(a.rows, a.n_items, b);          // uniform: a scalar load and two scalar selects
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (!a.src[k]) continue;
    const int n = a.floats[k];
    const float* __restrict__ s = a.src[k] + (size_t)r * n;
    float* __restrict__ d = a.dst[k] + (size_t)b * n;
    if (a.vec >> k & 1) {
      for (int i = threadIdx.x; i < (n >> 2); i += RR_THREADS) ((f4*)d)[i] = ((const f4*)s)[i];
    } else {
      for (int i = threadIdx.x; i < n; i += RR_THREADS) d[i] = s[i];
    }
  }
  if (threadIdx.x == 0) a.rows_ok[b] = r;
  if (b != 0) return;
  int bad = 0;
  for (int i = threadIdx.x; i < a.B; i += RR_THREADS) {
    const long long v = a.rows[i];
    bad |= v < 0 || v >= a.n_items;
  }
  bad = __syncthreads_or(bad);
  if (threadIdx.x == 0) *a.status = bad ? FTN_REFIT_ROWS_BAD : 0;
}

extern "C" int ftn_refit_rows_gather(const long long* rows_dev, int B, long long n_items, const float* tail_dev,
                                     int tail_floats, const float* y_dev, const float* mask_dev_or_null,
                                     const float* late_dev_or_null, int row_floats, float* tail_out_dev,
                                     float* y_out_dev, float* mask_out_dev_or_null, float* late_out_dev_or_null,
                                     long long* rows_ok_dev, int* status_dev, void* stream) {
  const char* who = "ftn_refit_rows_gather";
  FTN_CHECK_ARG(rows_dev && tail_dev && y_dev && tail_out_dev && y_out_dev && rows_ok_dev && status_dev,
                "%s: null pointer", who);
  FTN_CHECK_ARG(!mask_dev_or_null == !mask_out_dev_or_null && !late_dev_or_null == !late_out_dev_or_null,
                "%s: mask and late need a store and an output each, or neither", who);
  FTN_CHECK_ARG(B >= 1 && n_items >= 1 && tail_floats >= 1 && row_floats >= tail_floats,
                "%s: B=%d n_items=%lld tail_floats=%d row_floats=%d (all >= 1, tail_floats <= row_floats)", who, B,
                n_items, tail_floats, row_floats);
  FTN_CHECK_ARG((((uintptr_t)rows_dev | (uintptr_t)rows_ok_dev) & 7) == 0, "%s: rows and rows_ok must be 8-byte aligned",
                who);
  FTN_CHECK_ARG(rows_ok_dev + B <= rows_dev || rows_dev + B <= rows_ok_dev, "%s: rows_ok must not overlap rows", who);
  RefitRowsArgs a;
  a.rows = rows_dev; a.n_items = n_items; a.rows_ok = rows_ok_dev; a.status = status_dev; a.B = B; a.vec = 0;
  const float* src[4] = {tail_dev, y_dev, mask_dev_or_null, late_dev_or_null};
  float* dst[4] = {tail_out_dev, y_out_dev, mask_out_dev_or_null, late_out_dev_or_null};
  uintptr_t all = (uintptr_t)status_dev;
  for (int k = 0; k < 4; ++k) {
    a.src[k] = src[k]; a.dst[k] = dst[k]; a.floats[k] = k == 0 ? tail_floats : row_floats;
    const uintptr_t both = (uintptr_t)src[k] | (uintptr_t)dst[k];
    all |= both;
    if (src[k] && a.floats[k] % 4 == 0 && (both & 15) == 0) a.vec |= 1 << k;
  }
  FTN_CHECK_ARG((all & 3) == 0, "%s: stores, outputs and the status word must be 4-byte aligned", who);
  hipLaunchKernelGGL(k_refit_rows_gather, dim3((unsigned)B), dim3(RR_THREADS), 0, (hipStream_t)stream, a);
  FTN_CHECK_LAUNCH();
  return 0;
}
