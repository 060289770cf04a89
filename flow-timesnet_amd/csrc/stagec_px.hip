// Pixel-major stage C of the TimesBlock conv path (block.hip): the fused pointwise chain on the exact fp32 MFMA
// (k_mlp) and on the split 16-bit engines (k_mlp_bf, k_mlp_bf_u1).  The position-major form is stagec_pos.hip.
#include <stdlib.h>
#include "ftn_pw.h"
#include "ftn_mlp.h"

static const bool g_mlp_split = [] { const char* e = getenv("FTN_MLP_SPLIT"); return e == nullptr || e[0] != '0'; }();   // split refill (default on)

// ---------------------------------------------------------------- stage C
// g  = act(act(W_out1 m + b) + W_res1 x + b)       hidden, d_ff channels
// a' = W_in2 g + b ;  r = W_res2 g + b - x         the stacked output projection W_c
// One wave owns NPX 16-pixel units; the hidden dimension is walked in chunks of
// 64 channels (4 MFMA row tiles).  Per chunk the workgroup stages that chunk's
// weight fragments (lane-linear, pre-packed on the host: FtnPlan.w_cfrag) in LDS
// once for its 4 waves; layer 1 and the residual read their B fragments (m, x
// rows) straight from global/L2 with a one-step-ahead prefetch; the hidden
// accumulators then ARE the B fragments of the output projection, which
// accumulates across chunks in registers.  Nothing hidden-sized touches memory.
#define MLP_HT 2   // hidden row tiles per chunk (pack.py CHUNK_TILES)

// PRE: the B fragments of layer 1 (m rows, <= 3 K-chunks) and of the residual (x rows, <= 4
// K-chunks) do not depend on the hidden chunk, so they are loaded ONCE into registers and the
// chunk loop touches no global memory besides the weight DMA.
#define MLP_PRE_KM 3
#define MLP_PRE_CP 4
template <int ACT, bool XVEC, int NPX, int OTM, bool EXACT, bool PRE>
__global__ __launch_bounds__(256, (NPX >= 3 ? 2 : 1)) void k_mlp(MlpArgs a) {
  constexpr int HT = MLP_HT;
  extern __shared__ __attribute__((aligned(16))) float wl[];
  const FtnDesc* __restrict__ d = a.desc;
  const int N = a.B * d->total_px;
  stamp(a.dbg, a.dbg_cap, blockIdx.x, 0);
  if ((int)(blockIdx.x * 4 * 16 * NPX) >= N) return;            // whole workgroup beyond the live pixels
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 15, q = lane >> 4;
  const int n0 = (blockIdx.x * 4 + wave) * (16 * NPX);
  const bool active = n0 < N;                                    // wave-uniform; idle waves still stage + sync
  // Weight fragments reach LDS by DMA (global_load_lds_dwordx4, 1 KiB per wave instruction)
  // into two buffers: chunk hc+1 is requested right before the output-projection MFMAs of
  // chunk hc (the longest phase, no other memory traffic) and has landed by the barrier that
  // ends the chunk, so staging is off the critical path.
  const int bufsz = a.cfrag_per_chunk * 256;
  const int wv = __builtin_amdgcn_readfirstlane(wave);
  auto dma_chunk = [&](int hc, int buf) {
    const float* __restrict__ src = a.cfrag + (size_t)hc * bufsz;
    for (int piece = wv; piece < a.cfrag_per_chunk; piece += 4)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + (size_t)piece * 256 + lane * 4),
                                       (__attribute__((address_space(3))) void*)(wl + (size_t)buf * bufsz + (size_t)piece * 256),
                                       16, 0, 0);
  };
  dma_chunk(0, 0);                                               // lands while the pixels are decoded
  Px px[NPX];
#pragma unroll
  for (int u = 0; u < NPX; ++u) px[u] = decode_px16(d, a.x, a.B, a.L, a.C, n0 + 16 * u, j, N);
  const int FP = a.FP, KM = a.KM, CP = a.CP;
  const int nht = FP >> 4;
  const int nKM = a.nKM, nCP = a.nCP, n_ot = EXACT ? OTM : a.n_ot;
  const int offWr = HT * nKM, offWc = offWr + HT * nCP;
  f4 mpre[PRE ? MLP_PRE_KM : 1][NPX], xpre[PRE ? MLP_PRE_CP : 1][NPX];
  if (PRE) {
#pragma unroll
    for (int s = 0; s < MLP_PRE_KM; ++s)
#pragma unroll
      for (int u = 0; u < NPX; ++u)
        mpre[s][u] = s < nKM ? *(const f4*)(a.m + (size_t)px[u].n * KM + 16 * s + 4 * q) : f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < MLP_PRE_CP; ++s)
#pragma unroll
      for (int u = 0; u < NPX; ++u)
        xpre[s][u] = s < nCP ? load_x4<XVEC>(px[u].xrow, 16 * s + 4 * q, a.C) : f4{0.f, 0.f, 0.f, 0.f};
  }
  f4 oacc[OTM][NPX];
#pragma unroll
  for (int o = 0; o < OTM; ++o) {
    f4 bv = {0.f, 0.f, 0.f, 0.f};
    if (o < n_ot) bv = *(const f4*)(a.bc + 16 * o + 4 * q);
#pragma unroll
    for (int u = 0; u < NPX; ++u) oacc[o][u] = bv;
  }

  __syncthreads();
  stamp(a.dbg, a.dbg_cap, blockIdx.x, 1);
  for (int hc = 0; hc < a.n_hchunks; ++hc) {
    const float* __restrict__ wlane = wl + (size_t)(hc & 1) * bufsz + lane * 4;
    if (hc == 1) stamp(a.dbg, a.dbg_cap, blockIdx.x, 2);
    if (active) {
    f4 h[HT][NPX];
    // ---- z = W_out1 m + b   (or z = m)
    if (nKM > 0) {
#pragma unroll
      for (int t = 0; t < HT; ++t) {
        f4 bv = {0.f, 0.f, 0.f, 0.f};
        if (hc * HT + t < nht) bv = *(const f4*)(a.bo + 16 * (hc * HT + t) + 4 * q);
#pragma unroll
        for (int u = 0; u < NPX; ++u) h[t][u] = bv;
      }
      if (PRE) {
#pragma unroll
        for (int s = 0; s < MLP_PRE_KM; ++s) {
          if (s < nKM) {
#pragma unroll
            for (int t = 0; t < HT; ++t) {
              const f4 af = *(const f4*)(wlane + (t * nKM + s) * 256);
#pragma unroll
              for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int u = 0; u < NPX; ++u) h[t][u] = mfma16(af[e], mpre[s][u][e], h[t][u]);
            }
          }
        }
      } else {
        f4 bcur[NPX];
#pragma unroll
        for (int u = 0; u < NPX; ++u) bcur[u] = *(const f4*)(a.m + (size_t)px[u].n * KM + 4 * q);
        for (int s = 0; s < nKM; ++s) {
          const int sn = s + 1 < nKM ? s + 1 : s;
          f4 bnxt[NPX];
#pragma unroll
          for (int u = 0; u < NPX; ++u) bnxt[u] = *(const f4*)(a.m + (size_t)px[u].n * KM + 16 * sn + 4 * q);
#pragma unroll
          for (int t = 0; t < HT; ++t) {
            const f4 af = *(const f4*)(wlane + (t * nKM + s) * 256);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
              for (int u = 0; u < NPX; ++u) h[t][u] = mfma16(af[e], bcur[u][e], h[t][u]);
          }
#pragma unroll
          for (int u = 0; u < NPX; ++u) bcur[u] = bnxt[u];
        }
      }
    } else {
#pragma unroll
      for (int t = 0; t < HT; ++t)
#pragma unroll
        for (int u = 0; u < NPX; ++u) {
          f4 v = {0.f, 0.f, 0.f, 0.f};
          if (hc * HT + t < nht) v = *(const f4*)(a.m + (size_t)px[u].n * KM + 16 * (hc * HT + t) + 4 * q);
          h[t][u] = v;
        }
    }
    // ---- act, then + res1(x)                      (:652-654)
#pragma unroll
    for (int t = 0; t < HT; ++t)
#pragma unroll
      for (int u = 0; u < NPX; ++u) h[t][u] = act4<ACT>(h[t][u]);
    if (nCP > 0) {
#pragma unroll
      for (int t = 0; t < HT; ++t) {
        if (hc * HT + t < nht) {
          const f4 bv = *(const f4*)(a.br + 16 * (hc * HT + t) + 4 * q);
#pragma unroll
          for (int u = 0; u < NPX; ++u) h[t][u] += bv;
        }
      }
      if (PRE) {
#pragma unroll
        for (int s = 0; s < MLP_PRE_CP; ++s) {
          if (s < nCP) {
#pragma unroll
            for (int t = 0; t < HT; ++t) {
              const f4 af = *(const f4*)(wlane + (offWr + t * nCP + s) * 256);
#pragma unroll
              for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int u = 0; u < NPX; ++u) h[t][u] = mfma16(af[e], xpre[s][u][e], h[t][u]);
            }
          }
        }
      } else {
        f4 bcur[NPX];
#pragma unroll
        for (int u = 0; u < NPX; ++u) bcur[u] = load_x4<XVEC>(px[u].xrow, 4 * q, a.C);
        for (int s = 0; s < nCP; ++s) {
          const int sn = s + 1 < nCP ? s + 1 : s;
          f4 bnxt[NPX];
#pragma unroll
          for (int u = 0; u < NPX; ++u) bnxt[u] = load_x4<XVEC>(px[u].xrow, 16 * sn + 4 * q, a.C);
#pragma unroll
          for (int t = 0; t < HT; ++t) {
            const f4 af = *(const f4*)(wlane + (offWr + t * nCP + s) * 256);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
              for (int u = 0; u < NPX; ++u) h[t][u] = mfma16(af[e], bcur[u][e], h[t][u]);
          }
#pragma unroll
          for (int u = 0; u < NPX; ++u) bcur[u] = bnxt[u];
        }
      }
    } else {
#pragma unroll
      for (int t = 0; t < HT; ++t)
#pragma unroll
        for (int u = 0; u < NPX; ++u)
          if (hc * HT + t < nht) h[t][u] += load_x4<XVEC>(px[u].xrow, 16 * (hc * HT + t) + 4 * q, a.C);
    }
    // ---- mid activation                           (:753)
#pragma unroll
    for (int t = 0; t < HT; ++t)
#pragma unroll
      for (int u = 0; u < NPX; ++u) h[t][u] = act4<ACT>(h[t][u]);
    // ---- optional stores taken straight from the hidden tiles
    if (a.outG != nullptr || a.res2_ident) {
#pragma unroll
      for (int t = 0; t < HT; ++t) {
        if (hc * HT + t < nht) {
#pragma unroll
          for (int u = 0; u < NPX; ++u) {
            if (!px[u].ok) continue;
            const int ch = 16 * (hc * HT + t) + 4 * q;
            if (a.outG != nullptr) *(f4*)(a.outG + (size_t)px[u].n * FP + ch) = h[t][u];
            if (a.res2_ident)
              *(f4*)(a.outR + (size_t)px[u].n * CP + ch) = h[t][u] - load_x4<XVEC>(px[u].xrow, ch, a.C);
          }
        }
      }
    }
    // ---- request the next chunk's fragments, then the output projection: the hidden
    //      accumulators ARE the B fragments
    if (hc + 1 < a.n_hchunks) dma_chunk(hc + 1, (hc + 1) & 1);
#pragma unroll
    for (int t = 0; t < HT; ++t) {
#pragma unroll
      for (int o = 0; o < OTM; ++o) {
        if (EXACT || o < n_ot) {
          const f4 af = *(const f4*)(wlane + (offWc + t * n_ot + o) * 256);
#pragma unroll
          for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int u = 0; u < NPX; ++u) oacc[o][u] = mfma16(af[e], h[t][u][e], oacc[o][u]);
        }
      }
    }
    } else if (hc + 1 < a.n_hchunks) {
      dma_chunk(hc + 1, (hc + 1) & 1);
    }
    __syncthreads();   // everyone is done with this buffer and (vmcnt(0)) the next one has landed
  }
  stamp(a.dbg, a.dbg_cap, blockIdx.x, 3);
  if (!active) return;
  // ---- epilogue: a' tiles, then r = res2(g) - x tiles
#pragma unroll
  for (int o = 0; o < OTM; ++o) {
    if (EXACT || o < n_ot) {
#pragma unroll
      for (int u = 0; u < NPX; ++u) {
        if (!px[u].ok) continue;
        if (o < a.n_oa) {
          if (a.outA_p3 == 2) store_h2((__bf16*)a.outA + ((size_t)px[u].n * (a.AC >> 4) + o) * 32, q, oacc[o][u]);
          else if (a.outA_p3) store_p3((__bf16*)a.outA + ((size_t)px[u].n * (a.AC >> 4) + o) * 48, q, oacc[o][u]);
          else *(f4*)(a.outA + (size_t)px[u].n * a.AC + 16 * o + 4 * q) = oacc[o][u];
        } else {
          const int ch = 16 * (o - a.n_oa) + 4 * q;
          *(f4*)(a.outR + (size_t)px[u].n * CP + ch) = oacc[o][u] - load_x4<XVEC>(px[u].xrow, ch, a.C);
        }
      }
    }
  }
}

// ---------------------------------------------------------------- stage C, bf16x3 engine
// The same register-chained pointwise stage on the bf16 matrix pipe: every operand is three
// bf16 pieces and every K=32 slab is the six-product chain of k_conv_bf.  Layer-1 inputs
// (m: P3 rows written by the conv; x: split on load) are preloaded once; after the two
// GELUs the fp32 hidden accumulators of a 32-channel chunk (two row tiles) are split into
// pieces in registers and become the B operand of the output projection (the host packs
// the projection's K order to match the accumulator lane map).  The waves of a workgroup share
// each chunk's weight fragments, DMA-staged into LDS.
// 4-wave 128-pixel workgroups with a single weight buffer (2 x 66 KB would not fit twice), two per CU:
// VALU and MFMA work of a SIMD serialise on gfx950 (tools/ubench/mfma_valu.hip), so what a second
// workgroup buys is cover for the first one's prologue loads, chunk barriers, DMA waits and stores.
template <int ACT, bool XVEC, int OTM, bool EXACT, int NS>
__global__ __launch_bounds__(256, 2) void k_mlp_bf(MlpBfArgs a) {
  constexpr int NW = 4, NPX = 2;
  extern __shared__ __attribute__((aligned(16))) char wlb[];
  const FtnDesc* __restrict__ d = a.desc;
  const int N = a.B * d->total_px;
  stamp(a.dbg, a.dbg_cap, blockIdx.x, 0);
  if ((int)(blockIdx.x * NW * 16 * NPX) >= N) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 15, qa = lane >> 4;
  const int wv = __builtin_amdgcn_readfirstlane(wave);
  const int n0 = (blockIdx.x * NW + wave) * (16 * NPX);
  const bool active = n0 < N;
  const int bufsz = a.per_chunk * 3 * 1024;
  // the fragments of chunk hc -> the weight buffer
  auto dma_chunk = [&](int hc) {
    const __bf16* __restrict__ src = a.cfrag + (size_t)hc * a.per_chunk * 3 * 512;
    for (int piece = wv; piece < 3 * a.per_chunk; piece += NW)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + (size_t)piece * 512 + lane * 8),
                                       (__attribute__((address_space(3))) void*)(wlb + (size_t)piece * 1024),
                                       16, 0, 0);
  };
  // Prologue order matters: vmcnt retires in order, so whatever is issued before the pixel loads is
  // waited for with them.  Decode first (scalar loads only), then this wave's m / x rows, and only then
  // the chunk-0 weight DMA and the bias staging, which are not needed before the first barrier.
  Px px[NPX];
#pragma unroll
  for (int u = 0; u < NPX; ++u) px[u] = decode_px16(d, a.x, a.B, a.L, a.C, n0 + 16 * u, j, N);
  const int CP = a.CP;
  const int nsKM = a.nsKM, nsCP = a.nsCP, n_ot = EXACT ? OTM : a.n_ot;
  const int kmg = a.KM >> 4;                                  // 16-channel groups of m
  constexpr int NWP = PxFmt<NS>::NW;                          // weight pieces per fragment
  constexpr int PXE = PxFmt<NS>::ELEMS;                       // 16-bit elements per pixel and 16-channel group
  // B operands that do not depend on the hidden chunk
  bool range_bad = false;                                       // f16x2: a value left the fp16 range (ftn_common.h)
  bf8 mp[2][NPX][NS], xp[2][NPX][NS];
  f4 xraw[2][NPX][2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
#pragma unroll
    for (int u = 0; u < NPX; ++u) {
      const int grp = 2 * s + (qa >> 1);
      const __bf16* __restrict__ src = a.m + ((size_t)px[u].n * kmg + (grp < kmg ? grp : 0)) * PXE + (qa & 1) * 8;
#pragma unroll
      for (int pz = 0; pz < NS; ++pz) mp[s][u][pz] = *(const bf8*)(src + pz * 16);
      xraw[s][u][0] = s < nsCP ? load_x4<XVEC>(px[u].xrow, 32 * s + 8 * qa, a.C) : f4{0.f, 0.f, 0.f, 0.f};
      xraw[s][u][1] = s < nsCP ? load_x4<XVEC>(px[u].xrow, 32 * s + 8 * qa + 4, a.C) : f4{0.f, 0.f, 0.f, 0.f};
    }
  }
  __builtin_amdgcn_sched_barrier(0);
  dma_chunk(0);
  // biases of both hidden layers, zero-padded to whole chunks, in LDS behind the weight buffers
  const int FPc = a.n_hchunks * 32;
  float* __restrict__ bias_l = (float*)(wlb + (size_t)bufsz);
  for (int i = threadIdx.x; i < 2 * FPc; i += NW * 64) {
    const int c = i < FPc ? i : i - FPc;
    bias_l[i] = c < a.FP ? (i < FPc ? a.bo[c] : a.br[c]) : 0.f;
  }
#pragma unroll
  for (int s = 0; s < 2; ++s) {
#pragma unroll
    for (int u = 0; u < NPX; ++u) {
      const int grp = 2 * s + (qa >> 1);
      if (!(s < nsKM && grp < kmg)) {
#pragma unroll
        for (int pz = 0; pz < NS; ++pz)
#pragma unroll
          for (int e = 0; e < 8; ++e) mp[s][u][pz][e] = (__bf16)0.0f;
      }
      float xv[8];
#pragma unroll
      for (int e = 0; e < 4; ++e) { xv[e] = xraw[s][u][0][e]; xv[4 + e] = xraw[s][u][1][e]; }
      if (NS == 2) {
#pragma unroll
        for (int e = 0; e < 8; ++e) range_bad |= h2_bad(xv[e]);
      }
      split_pieces<NS>(xv, xp[s][u]);
    }
  }
  f4 oacc[OTM][NPX];
#pragma unroll
  for (int o = 0; o < OTM; ++o) {
    f4 bv = {0.f, 0.f, 0.f, 0.f};
    if (o < n_ot) bv = *(const f4*)(a.bc + 16 * o + 4 * qa);
#pragma unroll
    for (int u = 0; u < NPX; ++u) oacc[o][u] = bv;
  }
  __syncthreads();
  stamp(a.dbg, a.dbg_cap, blockIdx.x, 1);
  for (int hc = 0; hc < a.n_hchunks; ++hc) {
    if (hc == 1) stamp(a.dbg, a.dbg_cap, blockIdx.x, 2);
    const char* __restrict__ wl = wlb + lane * 16;
    // the biases come from LDS (staged once in the prologue), not from global memory
    f4 bo_t[2], br_t[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      bo_t[t] = *(const f4*)(bias_l + 16 * (hc * 2 + t) + 4 * qa);
      br_t[t] = *(const f4*)(bias_l + FPc + 16 * (hc * 2 + t) + 4 * qa);
    }
    f4 h[2][NPX];
    bf8 hp[NPX][NS];
    bf8 fa[NWP], fb[NWP];
    auto ldfrag = [&](int f, bf8 (&ap)[NWP]) {
#pragma unroll
      for (int pz = 0; pz < NWP; ++pz) ap[pz] = *(const bf8*)(wl + (size_t)(f * 3 + pz) * 1024);
    };
    auto gelu_u = [&](int t, int u, bool addbr) {
      if (NS == 2) {                                           // undo / apply the weight prescales (see MlpBfArgs)
        h[t][u] = act4<ACT>(h[t][u] * (addbr ? a.inv_o : a.inv_r));
        if (addbr) h[t][u] = h[t][u] * a.sc_r + br_t[t];
      } else {
        h[t][u] = act4<ACT>(h[t][u]);
        if (addbr) h[t][u] += br_t[t];
      }
    };
    auto split_u = [&](int u) {
      float hv[8];
#pragma unroll
      for (int e = 0; e < 4; ++e) { hv[e] = h[0][u][e]; hv[4 + e] = h[1][u][e]; }
      split_pieces<NS>(hv, hp[u]);
    };
    if (active) {
      // Statically scheduled chunk (KM <= 64, C <= 64: two K slabs each).  The 8 + 2*n_ot weight
      // fragments are walked in LDS order with a one-step-ahead register prefetch, and the
      // VALU work (GELU, piece splitting) of one row tile / pixel unit is placed in the same
      // scheduling region as MFMAs that do not depend on it, so both pipes stay busy although
      // the two waves of a SIMD run in lockstep between chunk barriers:
      //   f0 f1: L1(t0) | f2 f3: L1(t1) + G1(t0) | f4 f5: R(t0) + G1(t1) | f6 f7: R(t1) + G2(t0)
      //   G2(t1,u0) split(u0) | L2(u0) + G2(t1,u1) split(u1) | L2(u1)
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int u = 0; u < NPX; ++u) h[t][u] = bo_t[t];
      ldfrag(0, fa);
      // ---- L1(t0)
      ldfrag(1, fb); __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < NPX; ++u) h[0][u] = chain_bf<NS>(fa, mp[0][u], h[0][u]);
      ldfrag(2, fa); __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < NPX; ++u) h[0][u] = chain_bf<NS>(fb, mp[1][u], h[0][u]);
      // ---- L1(t1) + G1(t0)
      ldfrag(3, fb); __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < NPX; ++u) h[1][u] = chain_bf<NS>(fa, mp[0][u], h[1][u]);
      gelu_u(0, 0, true);
      ldfrag(4, fa); __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < NPX; ++u) h[1][u] = chain_bf<NS>(fb, mp[1][u], h[1][u]);
      gelu_u(0, 1, true);
      // ---- R(t0) + G1(t1)
      ldfrag(5, fb); __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < NPX; ++u) h[0][u] = chain_bf<NS>(fa, xp[0][u], h[0][u]);
      gelu_u(1, 0, true);
      ldfrag(6, fa); __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < NPX; ++u) h[0][u] = chain_bf<NS>(fb, xp[1][u], h[0][u]);
      gelu_u(1, 1, true);
      // ---- R(t1) + G2(t0)
      ldfrag(7, fb); __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < NPX; ++u) h[1][u] = chain_bf<NS>(fa, xp[0][u], h[1][u]);
      gelu_u(0, 0, false);
      ldfrag(8, fa); __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < NPX; ++u) h[1][u] = chain_bf<NS>(fb, xp[1][u], h[1][u]);
      gelu_u(0, 1, false);
      __builtin_amdgcn_sched_barrier(0);
      // ---- G2(t1,u0), split(u0)   (the only VALU stretch without an MFMA partner)
      gelu_u(1, 0, false);
      split_u(0);
      __builtin_amdgcn_sched_barrier(0);

      // ---- L2(u0) + G2(t1,u1), split(u1): fragments f = 8 .. 8+n_ot-1, ping-pong fa/fb
#pragma unroll
      for (int o = 0; o < OTM; ++o) {
        if (EXACT || o < n_ot) {
          if (o & 1) { ldfrag(8 + (o + 1 < n_ot ? o + 1 : 0), fa); __builtin_amdgcn_sched_barrier(0); oacc[o][0] = chain_bf<NS>(fb, hp[0], oacc[o][0]); }
          else       { ldfrag(8 + (o + 1 < n_ot ? o + 1 : 0), fb); __builtin_amdgcn_sched_barrier(0); oacc[o][0] = chain_bf<NS>(fa, hp[0], oacc[o][0]); }
          if (o == 0) gelu_u(1, 1, false);
          if (o == 1 || (n_ot == 1 && o == 0)) split_u(1);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      // ---- L2(u1): the wrap-around prefetch above left fragment 8 in the next register set
#pragma unroll
      for (int o = 0; o < OTM; ++o) {
        if (EXACT || o < n_ot) {
          const bool odd = ((n_ot + o) & 1) != 0;
          if (odd) { ldfrag(8 + (o + 1 < n_ot ? o + 1 : o), fa); __builtin_amdgcn_sched_barrier(0); oacc[o][1] = chain_bf<NS>(fb, hp[1], oacc[o][1]); }
          else     { ldfrag(8 + (o + 1 < n_ot ? o + 1 : o), fb); __builtin_amdgcn_sched_barrier(0); oacc[o][1] = chain_bf<NS>(fa, hp[1], oacc[o][1]); }
        }
      }
    }
    if (hc == 1) stamp(a.dbg, a.dbg_cap, blockIdx.x, 7);
    if (hc == 1 && a.dbg) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); stamp(a.dbg, a.dbg_cap, blockIdx.x, 5); }
    __syncthreads();
    if (hc == 1) stamp(a.dbg, a.dbg_cap, blockIdx.x, 4);
    if (hc + 1 < a.n_hchunks) {
      // single buffer: refill once every wave has left the chunk.  (Refilling in halves behind a
      // mid-chunk barrier hides the DMA but costs more in barrier skew than it saves: measured +5 %.)
      dma_chunk(hc + 1);
      __syncthreads();
    }
    if (hc == 1) stamp(a.dbg, a.dbg_cap, blockIdx.x, 6);
  }
  stamp(a.dbg, a.dbg_cap, blockIdx.x, 3);
  if (!active) { if (NS == 2) raise_range_flag(a.range_flag, range_bad); return; }
#pragma unroll
  for (int o = 0; o < OTM; ++o) {
    if (EXACT || o < n_ot) {
#pragma unroll
      for (int u = 0; u < NPX; ++u) {
        if (!px[u].ok) continue;
        if (o < a.n_oa) {
          const f4 av = NS == 2 ? oacc[o][u] * a.inv_a : oacc[o][u];
          if (NS == 2) range_bad |= h2_bad4(av);
          store_px<NS == 2 ? 2 : 3>(a.outA + ((size_t)px[u].n * (a.AC >> 4) + o) * PXE, qa, av);
        } else {
          const int ch = 16 * (o - a.n_oa) + 4 * qa;
          const f4 rv = NS == 2 ? oacc[o][u] * a.inv_r2 : oacc[o][u];
          *(f4*)(a.outR + (size_t)px[u].n * CP + ch) = rv - load_x4<XVEC>(px[u].xrow, ch, a.C);
        }
      }
    }
  }
  if (NS == 2) raise_range_flag(a.range_flag, range_bad);
}

// ---------------------------------------------------------------- stage C, bf16x3 engine, d_model 128
// The same chain for the reference's default pipeline shape (configs/default.yaml: d_model 128, d_ff 512,
// three kernels, ratio 4): nbr*mid = 96 = three K slabs of layer 1, d_model = 128 = four slabs of the
// residual, 6 + 8 = 14 output tiles.  With two 16-pixel units per wave that needs ~340 registers, so a wave
// owns ONE unit (oacc 56 + m pieces 36 + x pieces 48 registers) and the workgroup is 8 waves = 128 pixels;
// the 28 fragments of a chunk (84 KB) live in a single LDS buffer.  A fragment then feeds 6 MFMAs instead of
// 12 - which lands on the LDS read rate (tools/ubench/lds_patterns.hip) at about the time the SIMD needs
// for MFMA + GELU anyway.  The chunk is walked as one unrolled fragment sequence with a one-ahead prefetch.
// SKM / SCP = K=32 slabs of layer 1 / of the residual, OTM = output tiles: <3, 4, 14> is that shape; <2, 2, 7> is
// d_model 64 with three kernels of mid 16 (48 -> 64 K padding), where the smaller register footprint lets two
// 8-wave workgroups = four waves per SIMD share a CU (the two-unit k_mlp_bf above runs two).
// Two single-buffered 128-pixel workgroups per CU (other launch shapes measured slower: DESIGN.md section 4).
template <int ACT, bool XVEC, int NS, int SKM, int SCP, int OTM, bool SPLIT = false>
__global__ __launch_bounds__(512, 2) void k_mlp_bf_u1(MlpBfArgs a) {
  constexpr int NWV = 8;
  constexpr int NFR = 2 * SKM + 2 * SCP + OTM;
  constexpr int NL1 = 2 * SKM + 2 * SCP;        // fragments of layer 1 (+ residual); the other OTM are layer 2's
  extern __shared__ __attribute__((aligned(16))) char wlb[];
  const FtnDesc* __restrict__ d = a.desc;
  const int N = a.B * d->total_px;
  if ((int)(blockIdx.x * NWV * 16) >= N) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 15, qa = lane >> 4;
  const int wv = __builtin_amdgcn_readfirstlane(wave);
  const int n0 = (blockIdx.x * NWV + wave) * 16;
  const bool active = n0 < N;
  const int bufsz = NFR * 3 * 1024;
  auto dma_chunk = [&](int hc) {
    const __bf16* __restrict__ src = a.cfrag + (size_t)hc * NFR * 3 * 512;
    for (int piece = wv; piece < NFR * 3; piece += NWV)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + (size_t)piece * 512 + lane * 8),
                                       (__attribute__((address_space(3))) void*)(wlb + (size_t)piece * 1024), 16, 0, 0);
  };
  // SPLIT: LDS = [layer-1 fragments, two buffers][layer-2 fragments, one buffer][biases].  A chunk's layer-2 fragments
  // and the NEXT chunk's layer-1 fragments are requested at the top of the chunk and land while layer 1 runs; the
  // barrier between the layers waits (counted vmcnt) for the former only.  Two barriers per chunk as before, but no
  // wave ever waits for a refill it has just issued - that wait was 17 % of the launch (ablation).
  constexpr int l1sz = NL1 * 3 * 1024, l2sz = OTM * 3 * 1024;
  auto dma_l1 = [&](int hc, int buf) {
    const __bf16* __restrict__ src = a.cfrag + (size_t)hc * NFR * 3 * 512;
    char* dst = wlb + (size_t)buf * l1sz;
    for (int piece = wv; piece < NL1 * 3; piece += NWV)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + (size_t)piece * 512 + lane * 8),
                                       (__attribute__((address_space(3))) void*)(dst + (size_t)piece * 1024), 16, 0, 0);
  };
  auto dma_l2 = [&](int hc) {
    const __bf16* __restrict__ src = a.cfrag + ((size_t)hc * NFR + NL1) * 3 * 512;
    char* dst = wlb + 2 * l1sz;
    for (int piece = wv; piece < OTM * 3; piece += NWV)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + (size_t)piece * 512 + lane * 8),
                                       (__attribute__((address_space(3))) void*)(dst + (size_t)piece * 1024), 16, 0, 0);
  };
  const int n1_mine = (NL1 * 3 - wv + NWV - 1) / NWV;          // layer-1 pieces this wave requests per chunk
  const Px px = decode_px16(d, a.x, a.B, a.L, a.C, n0, j, N);
  const int CP = a.CP;
  const int kmg = a.KM >> 4;
  constexpr int NWP = PxFmt<NS>::NW;
  constexpr int PXE = PxFmt<NS>::ELEMS;
  bool range_bad = false;                                       // f16x2: a value left the fp16 range (ftn_common.h)
  bf8 mp[SKM][NS], xp[SCP][NS];
  f4 xraw[SCP][2];
#pragma unroll
  for (int s = 0; s < SKM; ++s) {
    const int grp = 2 * s + (qa >> 1);
    const __bf16* __restrict__ src = a.m + ((size_t)px.n * kmg + (grp < kmg ? grp : 0)) * PXE + (qa & 1) * 8;
#pragma unroll
    for (int pz = 0; pz < NS; ++pz) mp[s][pz] = *(const bf8*)(src + pz * 16);
  }
#pragma unroll
  for (int s = 0; s < SCP; ++s) {
    xraw[s][0] = load_x4<XVEC>(px.xrow, 32 * s + 8 * qa, a.C);
    xraw[s][1] = load_x4<XVEC>(px.xrow, 32 * s + 8 * qa + 4, a.C);
  }
  __builtin_amdgcn_sched_barrier(0);
  if (SPLIT) dma_l1(0, 0);
  else dma_chunk(0);
  const int FPc = a.n_hchunks * 32;
  float* __restrict__ bias_l = (float*)(wlb + (SPLIT ? (size_t)(2 * l1sz + l2sz) : (size_t)bufsz));
  for (int i = threadIdx.x; i < 2 * FPc; i += NWV * 64) {
    const int c = i < FPc ? i : i - FPc;
    bias_l[i] = c < a.FP ? (i < FPc ? a.bo[c] : a.br[c]) : 0.f;
  }
#pragma unroll
  for (int s = 0; s < SKM; ++s) {
    if (2 * s + (qa >> 1) >= kmg) {
#pragma unroll
      for (int pz = 0; pz < NS; ++pz)
#pragma unroll
        for (int e = 0; e < 8; ++e) mp[s][pz][e] = (__bf16)0.0f;
    }
  }
#pragma unroll
  for (int s = 0; s < SCP; ++s) {
    float xv[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) { xv[e] = xraw[s][0][e]; xv[4 + e] = xraw[s][1][e]; }
    if (NS == 2) {
#pragma unroll
      for (int e = 0; e < 8; ++e) range_bad |= h2_bad(xv[e]);
    }
    split_pieces<NS>(xv, xp[s]);
  }
  f4 oacc[OTM];
#pragma unroll
  for (int o = 0; o < OTM; ++o) oacc[o] = *(const f4*)(a.bc + 16 * o + 4 * qa);
  __syncthreads();
  if constexpr (SPLIT) {
    for (int hc = 0; hc < a.n_hchunks; ++hc) {
      const bool nxt = hc + 1 < a.n_hchunks;
      dma_l2(hc);                                    // last read in chunk hc - 1's layer 2 (every wave is past its end barrier)
      if (nxt) dma_l1(hc + 1, (hc + 1) & 1);         // that buffer was last read in chunk hc - 1's layer 1
      const char* __restrict__ wl1 = wlb + (size_t)(hc & 1) * l1sz + lane * 16;
      const char* __restrict__ wl2 = wlb + 2 * l1sz + lane * 16;
      f4 bo_t[2], br_t[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        bo_t[t] = *(const f4*)(bias_l + 16 * (hc * 2 + t) + 4 * qa);
        br_t[t] = *(const f4*)(bias_l + FPc + 16 * (hc * 2 + t) + 4 * qa);
      }
      f4 h[2] = {bo_t[0], bo_t[1]};
      bf8 hp[NS];
      bf8 fr[2][NWP];
      auto ldfrag = [&](int f, bf8 (&ap)[NWP]) {
        const char* __restrict__ base = f < NL1 ? wl1 + (size_t)f * 3 * 1024 : wl2 + (size_t)(f - NL1) * 3 * 1024;
#pragma unroll
        for (int pz = 0; pz < NWP; ++pz) ap[pz] = *(const bf8*)(base + (size_t)pz * 1024);
      };
      auto step = [&](int f) {
        if (f + 1 < NFR) ldfrag(f + 1, fr[(f + 1) & 1]);
        __builtin_amdgcn_sched_barrier(0);
        const bf8 (&cur)[NWP] = fr[f & 1];
        if (f < SKM) h[0] = chain_bf<NS>(cur, mp[f < SKM ? f : 0], h[0]);
        else if (f < 2 * SKM) h[1] = chain_bf<NS>(cur, mp[f < 2 * SKM ? f - SKM : 0], h[1]);
        else if (f < 2 * SKM + SCP) h[0] = chain_bf<NS>(cur, xp[f < 2 * SKM + SCP ? f - 2 * SKM : 0], h[0]);
        else if (f < NL1) h[1] = chain_bf<NS>(cur, xp[f < NL1 ? f - 2 * SKM - SCP : 0], h[1]);
        else oacc[f < NFR ? f - NL1 : 0] = chain_bf<NS>(cur, hp, oacc[f < NFR ? f - NL1 : 0]);
        if (f == SKM - 1) h[0] = NS == 2 ? act4<ACT>(h[0] * a.inv_o) * a.sc_r + br_t[0] : act4<ACT>(h[0]) + br_t[0];
        if (f == 2 * SKM - 1) h[1] = NS == 2 ? act4<ACT>(h[1] * a.inv_o) * a.sc_r + br_t[1] : act4<ACT>(h[1]) + br_t[1];
        if (f == 2 * SKM + SCP - 1) h[0] = act4<ACT>(NS == 2 ? h[0] * a.inv_r : h[0]);
        if (f == NL1 - 1) {
          h[1] = act4<ACT>(NS == 2 ? h[1] * a.inv_r : h[1]);
          float hv[8];
#pragma unroll
          for (int e = 0; e < 4; ++e) { hv[e] = h[0][e]; hv[4 + e] = h[1][e]; }
          split_pieces<NS>(hv, hp);
        }
        __builtin_amdgcn_sched_barrier(0);
      };
      if (active) {
        ldfrag(0, fr[0]);
#pragma unroll
        for (int f = 0; f < NL1 - 1; ++f) step(f);       // these steps read layer-1 fragments only (incl. the prefetch)
      }
      // layer 2's fragments have landed on every wave; the next chunk's layer-1 pieces (issued behind them) stay in flight
      barrier_keep_vm(nxt ? n1_mine : 0);
      if (active) {
#pragma unroll
        for (int f = NL1 - 1; f < NFR; ++f) step(f);     // the last layer-1 step prefetches the first layer-2 fragment
      }
      barrier_keep_vm(0);                              // every wave is done with both buffers; the next layer-1 set has landed
    }
  } else
  for (int hc = 0; hc < a.n_hchunks; ++hc) {
    const char* __restrict__ wl = wlb + lane * 16;
    f4 bo_t[2], br_t[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      bo_t[t] = *(const f4*)(bias_l + 16 * (hc * 2 + t) + 4 * qa);
      br_t[t] = *(const f4*)(bias_l + FPc + 16 * (hc * 2 + t) + 4 * qa);
    }
    if (active) {
      f4 h[2] = {bo_t[0], bo_t[1]};
      bf8 hp[NS];
      bf8 fr[2][NWP];                                  // fragment reads run one step ahead of their MFMAs
      auto ldfrag = [&](int f, bf8 (&ap)[NWP]) {
#pragma unroll
        for (int pz = 0; pz < NWP; ++pz) ap[pz] = *(const bf8*)(wl + (size_t)(f * 3 + pz) * 1024);
      };
      ldfrag(0, fr[0]);
#pragma unroll
      for (int f = 0; f < NFR; ++f) {
        if (f + 1 < NFR) ldfrag(f + 1, fr[(f + 1) & 1]);
        __builtin_amdgcn_sched_barrier(0);
        const bf8 (&cur)[NWP] = fr[f & 1];
        if (f < SKM) h[0] = chain_bf<NS>(cur, mp[f], h[0]);                         // layer 1, hidden tile 0
        else if (f < 2 * SKM) h[1] = chain_bf<NS>(cur, mp[f - SKM], h[1]);          // layer 1, hidden tile 1
        else if (f < 2 * SKM + SCP) h[0] = chain_bf<NS>(cur, xp[f - 2 * SKM], h[0]);               // + res1(x)
        else if (f < 2 * SKM + 2 * SCP) h[1] = chain_bf<NS>(cur, xp[f - 2 * SKM - SCP], h[1]);
        else oacc[f - 2 * SKM - 2 * SCP] = chain_bf<NS>(cur, hp, oacc[f - 2 * SKM - 2 * SCP]);    // a' | res2
        // act, then the residual adds on; NS == 2 undoes / applies the weight prescales (see MlpBfArgs)
        if (f == SKM - 1) h[0] = NS == 2 ? act4<ACT>(h[0] * a.inv_o) * a.sc_r + br_t[0] : act4<ACT>(h[0]) + br_t[0];
        if (f == 2 * SKM - 1) h[1] = NS == 2 ? act4<ACT>(h[1] * a.inv_o) * a.sc_r + br_t[1] : act4<ACT>(h[1]) + br_t[1];
        if (f == 2 * SKM + SCP - 1) h[0] = act4<ACT>(NS == 2 ? h[0] * a.inv_r : h[0]);   // TimesBlock's mid activation
        if (f == 2 * SKM + 2 * SCP - 1) {
          h[1] = act4<ACT>(NS == 2 ? h[1] * a.inv_r : h[1]);
          float hv[8];
#pragma unroll
          for (int e = 0; e < 4; ++e) { hv[e] = h[0][e]; hv[4 + e] = h[1][e]; }
          split_pieces<NS>(hv, hp);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    __syncthreads();
    if (hc + 1 < a.n_hchunks) {
      dma_chunk(hc + 1);
      __syncthreads();
    }
  }
  if (active && px.ok && NS == 2) {
#pragma unroll
    for (int o = 0; o < OTM; ++o)
      if (o < a.n_oa) range_bad |= h2_bad4(oacc[o] * a.inv_a);
  }
  if (NS == 2) raise_range_flag(a.range_flag, range_bad);
  if (!active || !px.ok) return;
#pragma unroll
  for (int o = 0; o < OTM; ++o) {
    if (o < a.n_oa) {
      store_px<NS == 2 ? 2 : 3>(a.outA + ((size_t)px.n * (a.AC >> 4) + o) * PXE, qa, NS == 2 ? oacc[o] * a.inv_a : oacc[o]);
    } else {
      const int ch = 16 * (o - a.n_oa) + 4 * qa;
      const f4 rv = NS == 2 ? oacc[o] * a.inv_r2 : oacc[o];
      *(f4*)(a.outR + (size_t)px.n * CP + ch) = a.r_keeps_x ? rv : rv - load_x4<XVEC>(px.xrow, ch, a.C);
    }
  }
}

template <int ACT, int NS, int SKM, int SCP, int OTM, bool SPLIT = false>
static int launch_mlp_bf_u1w(MlpBfArgs ma, bool xvec, long long Nmax, hipStream_t st) {
  ma.dbg = nullptr; ma.dbg_cap = 0;
  const size_t lds = (SPLIT ? (size_t)(2 * (2 * SKM + 2 * SCP) + OTM) * 3 * 1024
                            : (size_t)ma.per_chunk * 3 * 1024) + (size_t)ma.n_hchunks * 32 * 2 * sizeof(float);
  if (lds > 160 * 1024) { ftn_set_error("stage C needs %zu B of LDS", lds); return -1; }
  const int nblk = (int)((Nmax + 8 * 16 - 1) / (8 * 16));
  hipError_t e = xvec ? hipFuncSetAttribute((const void*)k_mlp_bf_u1<ACT, true, NS, SKM, SCP, OTM, SPLIT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)
                      : hipFuncSetAttribute((const void*)k_mlp_bf_u1<ACT, false, NS, SKM, SCP, OTM, SPLIT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) { ftn_set_error("hipFuncSetAttribute(k_mlp_bf_u1): %s", hipGetErrorString(e)); return (int)e; }
  if (xvec) hipLaunchKernelGGL((k_mlp_bf_u1<ACT, true, NS, SKM, SCP, OTM, SPLIT>), dim3(nblk), dim3(512), lds, st, ma);
  else hipLaunchKernelGGL((k_mlp_bf_u1<ACT, false, NS, SKM, SCP, OTM, SPLIT>), dim3(nblk), dim3(512), lds, st, ma);
  FTN_CHECK_LAUNCH();
  return 0;
}

template <int ACT, int NS, int SKM, int SCP, int OTM>
static int launch_mlp_bf_u1(const MlpBfArgs& ma, bool xvec, long long Nmax, hipStream_t st) {
  // split refill where two workgroups' LDS still fit a CU (or, for the d_model-128 shape, one does)
  if (g_mlp_split && ma.per_chunk == 2 * SKM + 2 * SCP + OTM &&
      (size_t)(2 * (2 * SKM + 2 * SCP) + OTM) * 3 * 1024 + (size_t)ma.n_hchunks * 256 <= (OTM <= 7 ? 80 : 160) * 1024)
    return launch_mlp_bf_u1w<ACT, NS, SKM, SCP, OTM, true>(ma, xvec, Nmax, st);
  return launch_mlp_bf_u1w<ACT, NS, SKM, SCP, OTM>(ma, xvec, Nmax, st);
}

template <int ACT, bool XVEC, int NPX, int OTM, bool EXACT, bool PRE>
static int launch_mlp_t(MlpArgs ma, long long Nmax, hipStream_t st) {
  ma.dbg = ftn_stamp_buf(2, &ma.dbg_cap);
  const size_t lds = (size_t)ma.cfrag_per_chunk * 1024 * 2;   // double-buffered
  if (lds > 160 * 1024) { ftn_set_error("stage C needs %zu B of LDS for two hidden chunks", lds); return -1; }
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)k_mlp<ACT, XVEC, NPX, OTM, EXACT, PRE>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) { ftn_set_error("hipFuncSetAttribute(k_mlp): %s", hipGetErrorString(e)); return (int)e; }
  }
  const int per = 16 * NPX * 4;
  const int nblk = (int)((Nmax + per - 1) / per);
  hipLaunchKernelGGL((k_mlp<ACT, XVEC, NPX, OTM, EXACT, PRE>), dim3(nblk), dim3(256), lds, st, ma);
  FTN_CHECK_LAUNCH();
  return 0;
}

template <int ACT, bool XVEC>
static int launch_mlp_x(const MlpArgs& ma, long long Nmax, hipStream_t st) {
  const bool pre = ma.nKM <= MLP_PRE_KM && ma.nCP <= MLP_PRE_CP;
  if (ma.n_ot == 7 && pre) return launch_mlp_t<ACT, XVEC, 3, 7, true, true>(ma, Nmax, st);   // d_model 64, mid 16, 3 kernels
  if (ma.n_ot <= 8) {
    if (pre) return launch_mlp_t<ACT, XVEC, 3, 8, false, true>(ma, Nmax, st);
    return launch_mlp_t<ACT, XVEC, 3, 8, false, false>(ma, Nmax, st);
  }
  if (ma.n_ot == 14) return launch_mlp_t<ACT, XVEC, 2, 14, true, false>(ma, Nmax, st);        // d_model 128, mid 32, 3 kernels
  return launch_mlp_t<ACT, XVEC, 2, 16, false, false>(ma, Nmax, st);
}

template <int ACT, bool XVEC, int OTM, bool EXACT, int NS>
static int launch_mlp_bf_t(MlpBfArgs ma, long long Nmax, hipStream_t st) {
  // 4-wave workgroups, two per CU (an 8-wave double-buffered form measured 425 us against 360 us at the bench shape)
  ma.dbg = ftn_stamp_buf(2, &ma.dbg_cap);
  const size_t lds = (size_t)ma.per_chunk * 3 * 1024 + (size_t)ma.n_hchunks * 32 * 2 * sizeof(float);
  hipError_t e = hipFuncSetAttribute((const void*)k_mlp_bf<ACT, XVEC, OTM, EXACT, NS>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) { ftn_set_error("hipFuncSetAttribute(k_mlp_bf): %s", hipGetErrorString(e)); return (int)e; }
  const int px_wg = 4 * 32;
  const int nblk = (int)((Nmax + px_wg - 1) / px_wg);
  hipLaunchKernelGGL((k_mlp_bf<ACT, XVEC, OTM, EXACT, NS>), dim3(nblk), dim3(256), lds, st, ma);
  FTN_CHECK_LAUNCH();
  return 0;
}

template <int ACT, int NS>
static int launch_mlp_bf(const MlpBfArgs& ma, bool xvec, long long Nmax, hipStream_t st) {
  if (ma.n_ot == 7) {
    if (xvec) return launch_mlp_bf_t<ACT, true, 7, true, NS>(ma, Nmax, st);
    return launch_mlp_bf_t<ACT, false, 7, true, NS>(ma, Nmax, st);
  }
  if (xvec) return launch_mlp_bf_t<ACT, true, 8, false, NS>(ma, Nmax, st);
  return launch_mlp_bf_t<ACT, false, 8, false, NS>(ma, Nmax, st);
}

int ftn_launch_mlp(const MlpArgs& ma, int act, bool xvec, long long Nmax, hipStream_t st) {
  if (ma.cfrag_per_chunk != MLP_HT * (ma.nKM + ma.nCP + ma.n_ot)) { ftn_set_error("plan/cfrag layout mismatch"); return -1; }
  if (act == 1) return xvec ? launch_mlp_x<1, true>(ma, Nmax, st) : launch_mlp_x<1, false>(ma, Nmax, st);
  return xvec ? launch_mlp_x<0, true>(ma, Nmax, st) : launch_mlp_x<0, false>(ma, Nmax, st);
}

template <int ACT, int NS>
static int launch_mlp_bf_form(const MlpBfArgs& mb, int form, bool xvec, long long Nmax, hipStream_t st) {
  // one 16-pixel unit per wave (see k_mlp_bf_u1): the d_model-128 shape, and d_model 64 with four waves per SIMD
  if (form == FTN_FORM_C_MLP_BF_C128) return launch_mlp_bf_u1<ACT, NS, 3, 4, 14>(mb, xvec, Nmax, st);
  if (form == FTN_FORM_C_MLP_BF_U1) return launch_mlp_bf_u1<ACT, NS, 2, 2, 7>(mb, xvec, Nmax, st);
  return launch_mlp_bf<ACT, NS>(mb, xvec, Nmax, st);
}

template <int ACT>
static int launch_mlp_bf_act(const MlpBfArgs& mb, int form, int nsplit, bool xvec, long long Nmax, hipStream_t st) {
  if (nsplit == 3) return launch_mlp_bf_form<ACT, 3>(mb, form, xvec, Nmax, st);
  if (nsplit == 2) return launch_mlp_bf_form<ACT, 2>(mb, form, xvec, Nmax, st);
  return launch_mlp_bf_form<ACT, 1>(mb, form, xvec, Nmax, st);
}

int ftn_launch_mlp_bf(const MlpBfArgs& mb, int form, int act, int nsplit, bool xvec, long long Nmax, hipStream_t st) {
  return act == 1 ? launch_mlp_bf_act<1>(mb, form, nsplit, xvec, Nmax, st) : launch_mlp_bf_act<0>(mb, form, nsplit, xvec, Nmax, st);
}
