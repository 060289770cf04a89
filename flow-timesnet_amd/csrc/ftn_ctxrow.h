// The wave-per-row arithmetic of a context vector (context.hip: k_context_rows; latefit.hip: the late-bias head for a
// refit): the butterfly sum, torch's affine LayerNorm of up to CTX_MAX values held four to a lane, and the FMA chain of
// a dot product.  Both files include this header so that the late bias has the same bits whichever kernel forms it.
#pragma once

#define CTX_MAX 256          // ctx, F, Ws, Ed
#define CTX_SLOTS 4          // CTX_MAX / 64: element lane + 64 j of a row vector lives in slot j of lane `lane`

// Sum over the 64 lanes by an xor butterfly: every lane ends with the same bits (fp32 addition commutes, and the two
// partners of a step hold the two operands of the same addition).
__device__ __forceinline__ float wave_sum(float s) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
  return s;
}

// Affine LayerNorm, as torch computes it, of the n <= 256 values v[j] = element lane + 64 j: the mean, then the
// biased variance of the centred values, 1 / sqrt(var + eps), gamma, beta.  Called by all 64 lanes.
__device__ __forceinline__ void wave_layernorm(float (&v)[CTX_SLOTS], int n, int lane, const float* __restrict__ g,
                                               const float* __restrict__ b, float eps) {
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < CTX_SLOTS; ++j)
    if (lane + 64 * j < n) s += v[j];
  const float mean = wave_sum(s) / (float)n;
  float ss = 0.f;
#pragma unroll
  for (int j = 0; j < CTX_SLOTS; ++j)
    if (lane + 64 * j < n) {
      v[j] -= mean;
      ss = fmaf(v[j], v[j], ss);
    }
  const float rstd = 1.0f / sqrtf(wave_sum(ss) / (float)n + eps);
#pragma unroll
  for (int j = 0; j < CTX_SLOTS; ++j) {
    const int k = lane + 64 * j;
    if (k < n) v[j] = fmaf(v[j] * rstd, g[k], b[k]);
  }
}

// sum_k w[k] v[k], k ascending, one FMA chain from +0
__device__ __forceinline__ float dot_chain(const float* __restrict__ w, const float* v, int n) {
  float acc = 0.f;
  for (int k = 0; k < n; ++k) acc = fmaf(w[k], v[k], acc);
  return acc;
}
