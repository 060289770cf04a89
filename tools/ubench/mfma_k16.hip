// Issue interval of the K=16 MFMAs (v_mfma_f32_16x16x16_bf16 / _f16) vs the K=32 ones on gfx950, with four
// independent accumulators (the issue rate) and with one (the dependent chain of a piece product, chain_bf).
//   hipcc -O3 --offload-arch=gfx950 tools/ubench/mfma_k16.hip -o tools/ubench/mfma_k16
#include <hip/hip_runtime.h>
#include <stdio.h>
typedef float f4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf8 __attribute__((ext_vector_type(8)));
typedef short s4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf4 __attribute__((ext_vector_type(4)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));

// F16: 0 bf16, 1 fp16.  NACC: accumulators the 16 MFMAs of one trip rotate over (a power of two).
template <int K, int F16, int NACC>
__global__ void k(float* out, unsigned long long* cyc, int iters) {
  const int lane = threadIdx.x & 63;
  bf8 a8, b8; bf4 a4, b4;
  h8 ha8, hb8; h4 ha4, hb4;
  for (int e = 0; e < 8; ++e) {
    a8[e] = (__bf16)(0.001f * (lane + e)); b8[e] = (__bf16)(0.002f * (lane - e));
    ha8[e] = (_Float16)(0.001f * (lane + e)); hb8[e] = (_Float16)(0.002f * (lane - e));
  }
  for (int e = 0; e < 4; ++e) { a4[e] = a8[e]; b4[e] = b8[e]; ha4[e] = ha8[e]; hb4[e] = hb8[e]; }
  f4 acc[NACC];
  for (int c = 0; c < NACC; ++c) acc[c] = f4{0.f, 0.f, 0.f, 0.f};
  const unsigned long long t0 = __builtin_amdgcn_s_memtime();
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      f4& c = acc[i & (NACC - 1)];
      if (K == 32 && F16 == 0) c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a8, b8, c, 0, 0, 0);
      else if (K == 32) c = __builtin_amdgcn_mfma_f32_16x16x32_f16(ha8, hb8, c, 0, 0, 0);
      else if (F16 == 0) c = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(s4, a4), __builtin_bit_cast(s4, b4), c, 0, 0, 0);
      else c = __builtin_amdgcn_mfma_f32_16x16x16f16(ha4, hb4, c, 0, 0, 0);
    }
  }
  const unsigned long long t1 = __builtin_amdgcn_s_memtime();
  float s = 0.f;
  for (int c = 0; c < NACC; ++c) s += acc[c][0] + acc[c][1] + acc[c][2] + acc[c][3];
  out[threadIdx.x] = s;
  if (threadIdx.x == 0) *cyc = t1 - t0;
}

template <int K, int F16, int NACC>
void run() {
  float* out; unsigned long long* cyc; unsigned long long h;
  (void)hipMalloc(&out, 4096); (void)hipMalloc(&cyc, 8);
  for (int r = 0; r < 2; ++r) hipLaunchKernelGGL((k<K, F16, NACC>), dim3(1), dim3(64), 0, 0, out, cyc, 2000);
  (void)hipDeviceSynchronize();
  (void)hipMemcpy(&h, cyc, 8, hipMemcpyDeviceToHost);
  printf("v_mfma_f32_16x16x%d %s, %d accumulator%s: %.2f cycles per MFMA\n", K, F16 ? "f16 " : "bf16", NACC,
         NACC > 1 ? "s" : " ", (double)h / 2000 / 16);
  (void)hipFree(out); (void)hipFree(cyc);
}
int main() {
  run<32, 0, 4>(); run<16, 0, 4>(); run<32, 1, 4>(); run<16, 1, 4>();
  run<32, 0, 1>(); run<16, 0, 1>(); run<32, 1, 1>(); run<16, 1, 1>();
  return 0;
}
