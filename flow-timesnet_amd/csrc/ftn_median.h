// Lower median over channels (torch.median: sorted[(C - 1) / 2]) inside one wave: ONE compare-exchange step and ONE
// bitonic network for every kernel of spectrum.hip.
//
// A row's values sit in V registers per lane (element index 64 i + lane, +inf beyond C; V = 1, 2, 4 for C <= 64, 128,
// 256) and are sorted ascending by the bitonic network of 64 V elements: 21 / 28 / 36 compare-exchange steps instead of
// a C x C rank count.  NR independent rows share one instruction stream: the dependent steps of a single sort (each a
// cross-lane move) would leave the wave waiting on its own latency chain, and every workgroup of a launch reaches
// this phase at the same time.  Values are only permuted - NaN-free, non-negative amplitudes - so the median is the
// same bits whatever V and NR a caller picks.  A row that holds a NaN (one NaN sample of x makes its channel NaN in
// every bin) reads NaN, as torch.median does: the network itself would lose it.
#pragma once
#include <math.h>
#include "ftn_common.h"

// lane ^ J partner value without the LDS crossbar where DPP can do it: J = 1, 2 are quad permutes, J = 8 a 16-lane row
// rotate, J = 4 two bank-masked row shifts (banks = groups of 4 lanes); J = 16, 32 go through ds_bpermute.  18 of the 21
// steps of a 64-element sort then cost VALU latency instead of LDS latency.  A raw v_mov_b32_dpp: hipcc wraps
// __builtin_amdgcn_update_dpp in a copy and a canonicalising v_max.
template <int J>
__device__ __forceinline__ float lane_partner(float v) {
  float o;
  if constexpr (J == 1) asm volatile("v_mov_b32_dpp %0, %1 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf" : "=v"(o) : "v"(v));
  else if constexpr (J == 2) asm volatile("v_mov_b32_dpp %0, %1 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf" : "=v"(o) : "v"(v));
  else if constexpr (J == 8) asm volatile("v_mov_b32_dpp %0, %1 row_ror:8 row_mask:0xf bank_mask:0xf" : "=v"(o) : "v"(v));
  else if constexpr (J == 4)
    asm volatile("v_mov_b32_dpp %0, %1 row_shl:4 row_mask:0xf bank_mask:0x5\n\t"
                 "v_mov_b32_dpp %0, %1 row_shr:4 row_mask:0xf bank_mask:0xa" : "=&v"(o) : "v"(v));
  else o = __shfl_xor(v, J);
  return o;
}

// The compare-exchange of stage K at lane distance J < 64 on one register of NR rows, three issue slots per value
// (min + max + select on update_dpp costs eight): the partner move above and ONE v_med3_f32 against -inf (keep the
// smaller) or +inf (keep the larger) - a per-lane constant that depends on the step only and is shared by the rows.
// DESC flips the direction: the register holds elements whose index has bit K set (K >= 64 never shows in a lane).
template <int K, int J, int NR, bool DESC>
__device__ __forceinline__ void bitonic_step(float (&v)[NR], int lane) {
  const bool keepmin = (((lane & K) == 0) == ((lane & J) == 0)) != DESC;
  const float sel = keepmin ? -INFINITY : INFINITY;
  float o[NR];
  // a DPP read needs two wait states after the VALU write of its source, and inline asm is opaque to hipcc's hazard
  // pass: ONE s_nop 1 in front of the step's DPP group (fenced so nothing that writes v[] can slip in behind it)
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (J < 16) asm volatile("s_nop 1");
#pragma unroll
  for (int r = 0; r < NR; ++r) o[r] = lane_partner<J>(v[r]);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int r = 0; r < NR; ++r) v[r] = __builtin_amdgcn_fmed3f(v[r], o[r], sel);
}

// Steps (K, J), (K, J / 2), .. (K, 1), then stage 2 K from distance K down, up to stage 64 V.  Register i runs
// descending in stage K when its elements have bit K set: ((64 i) & K) != 0, a constant once the loop is unrolled.
// Distances of 64 and 128 pair whole registers of a lane.
template <int V, int NR, int K, int J>
__device__ __forceinline__ void bitonic_from(float (&v)[V][NR], int lane) {
  if constexpr (K <= 64 * V) {
    if constexpr (J >= 64) {
      constexpr int di = J >> 6;
#pragma unroll
      for (int i = 0; i < V; ++i) {
        if ((i & di) != 0) continue;
        const bool up = ((64 * i) & K) == 0;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
          const float lo = fminf(v[i][r], v[i | di][r]), hi = fmaxf(v[i][r], v[i | di][r]);
          v[i][r] = up ? lo : hi;
          v[i | di][r] = up ? hi : lo;
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < V; ++i) {
        if (((64 * i) & K) != 0) bitonic_step<K, J, NR, true>(v[i], lane);
        else bitonic_step<K, J, NR, false>(v[i], lane);
      }
    }
    if constexpr (J > 1) bitonic_from<V, NR, K, J / 2>(v, lane);
    else bitonic_from<V, NR, 2 * K, K>(v, lane);
  }
}

// m[r] = lower median of the C <= 64 V values base[r * stride + 0 .. C), r < NR; every lane of the wave gets it.
template <int V, int NR>
__device__ __forceinline__ void wave_lower_median_rows(const float* __restrict__ base, size_t stride, int C, int lane,
                                                       float (&m)[NR]) {
  float v[V][NR];
#pragma unroll
  for (int i = 0; i < V; ++i)
#pragma unroll
    for (int r = 0; r < NR; ++r) v[i][r] = 64 * i + lane < C ? base[r * stride + 64 * i + lane] : INFINITY;
  // torch.median propagates NaN; v_med3_f32 drops it (and hands its partner the +-inf selector instead).  Lanes that
  // hold one in any row: one unordered compare (v_cmp_u_f32) per TWO values, which is all a NaN-free call pays
  unsigned long long anynan = 0;
#pragma unroll
  for (int j = 0; j < V * NR; j += 2) {
    const float a = v[j / NR][j % NR], b = j + 1 < V * NR ? v[(j + 1) / NR][(j + 1) % NR] : a;
    anynan |= __builtin_amdgcn_ballot_w64(__builtin_isunordered(a, b));
  }
  bitonic_from<V, NR, 2, 1>(v, lane);
  const int t = (C - 1) >> 1;
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    float s = v[0][r];                                   // register t / 64 (wave-uniform), then its lane t % 64
#pragma unroll
    for (int i = 1; i < V; ++i)
      if ((t >> 6) == i) s = v[i][r];
    m[r] = __shfl(s, t & 63);
  }
  if (anynan != 0) {                                     // wave-uniform and rare: which rows
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      bool bad = false;
      for (int c = lane; c < C; c += 64) bad |= base[r * stride + c] != base[r * stride + c];
      if (__builtin_amdgcn_ballot_w64(bad) != 0) m[r] = NAN;
    }
  }
}
