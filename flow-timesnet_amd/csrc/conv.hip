// Stages B and D of the TimesBlock conv path (block.hip): the grouped k x k convolution on the exact fp32 MFMA
// (k_conv) and on the split 16-bit engines (k_conv_bf, k_conv_bf_fast), with their launch geometry.
#include <stdlib.h>
#include "ftn_conv.h"
#include "ftn_conv_split.h"
#include "ftn_conv_walk.h"
#include "ftn_mlp.h"

static const bool g_conv_generic = [] { const char* e = getenv("FTN_CONV_GENERIC"); return e != nullptr && e[0] == '1'; }();  // experiment switch
// 0: the fast path shares out a branch's rows equally, tile switches uncharged (A/B runs and tests; default on)
static const bool g_conv_walk = [] { const char* e = getenv("FTN_CONV_WALK"); return e == nullptr || e[0] != '0'; }();
// What a workgroup of k_conv_bf_fast pays for walking on into the next tile, in the k-cycle unit of ftn_conv_split's
// row cost: workgroups with the same rows end 9.4 k (7x7) to 12 k (3x3) cycles later when they cross a tile boundary
// (tools/stamps.py)
#define FTN_CONV_SWITCH_KCYC 10.0

// ---------------------------------------------------------------- tile and pixel bookkeeping of the three kernels
// One conv tile of the per-row tile list: its period group, the group's grid, the tile inside it and the staged
// region = tile + halo, clipped to the grid.
struct ConvTile {
  int g;                                 // period group
  int p, cycles, P;                      // grid: columns (the period), rows, pixels
  int r0, c0, th, tw, npx, nunits;       // tile: origin, size, pixels, 16-pixel units
  int R0, C0, RW, RH;                    // staged region: origin, width, height
  // staged-region pixel sp (row-major) -> grid pixel = window position t (fold, :1041-1046); sp / RW by reciprocal
  __device__ __forceinline__ int grid_px(int sp, float inv_rw) const {
    const int rr = (int)(((float)sp + 0.5f) * inv_rw), cx = sp - rr * RW;
    return (R0 + rr) * p + C0 + cx;
  }
};

// tile bx of the descriptor's tile list for a kernel with halo (hy, hx).  G = d->n_groups, which the split-engine
// kernels read once in front of their tile loops (inside, behind the output stores, it is a vector load per tile)
__device__ __forceinline__ ConvTile conv_tile(const FtnDesc* __restrict__ d, int G, int bx, int hy, int hx) {
  ConvTile t;
  t.g = 0;
  for (int gg = 1; gg < G; ++gg)
    if (bx >= d->g_tile_off[gg]) t.g = gg;
  const int tix = bx - d->g_tile_off[t.g];
  const int ntx = d->g_ntx[t.g];
  const int ty = tix / ntx, tx = tix - ty * ntx;
  t.p = d->g_period[t.g]; t.cycles = d->g_cycles[t.g];
  t.P = d->g_px_off[t.g + 1] - d->g_px_off[t.g];
  t.r0 = ty * d->g_th[t.g]; t.c0 = tx * d->g_tw[t.g];
  t.th = min(d->g_th[t.g], t.cycles - t.r0); t.tw = min(d->g_tw[t.g], t.p - t.c0);
  t.npx = t.th * t.tw; t.nunits = (t.npx + 15) >> 4;
  const int R1 = min(t.cycles, t.r0 + t.th + hy), C1 = min(t.p, t.c0 + t.tw + hx);
  t.R0 = max(0, t.r0 - hy); t.C0 = max(0, t.c0 - hx);
  t.RW = C1 - t.C0; t.RH = R1 - t.R0;
  return t;
}

// grid pixel tpx of an input with one row per window position (bt_L > 0, ConvArgs.bt_L) is the shared pad row
__device__ __forceinline__ bool conv_pad_row(int bt_L, int tpx) { return bt_L > 0 && tpx >= bt_L; }

// Pixel idx of a tile (row-major; a lane's idx may lie past the tile: ok = false, it then stands on pixel 0 with
// empty masks): grid position (ri, ci) and the kernel taps that fall inside the grid, as a row and a column mask.
struct ConvPixel { int ri, ci; bool ok; unsigned rm, cm; };

__device__ __forceinline__ ConvPixel conv_pixel(const ConvTile& t, int idx, float inv_tw, int kh, int kw) {
  ConvPixel px;
  px.ok = idx < t.npx;
  if (!px.ok) idx = 0;
  // idx / tw by reciprocal: exact for idx < 2^20 because (idx + 0.5) / tw is never an integer
  const int r = (int)(((float)idx + 0.5f) * inv_tw), c = idx - r * t.tw;
  px.ri = t.r0 + r; px.ci = t.c0 + c;
  const int hy = kh >> 1, hx = kw >> 1;
  const unsigned kmh = (1u << kh) - 1u, kmw = (1u << kw) - 1u;
  // taps dy with 0 <= ri + dy - hy < cycles are the bits [lo, hi) of the row mask (same for columns)
  const int rlo = max(0, hy - px.ri), rhi = min(kh, t.cycles + hy - px.ri);
  const int clo = max(0, hx - px.ci), chi = min(kw, t.p + hx - px.ci);
  const unsigned rm = (rhi > rlo) ? ((kmh >> (kh - rhi)) & (kmh << rlo)) & kmh : 0u;
  const unsigned cm = (chi > clo) ? ((kmw >> (kw - chi)) & (kmw << clo)) & kmw : 0u;
  px.rm = px.ok ? rm : 0u;
  px.cm = px.ok ? cm : 0u;
  return px;
}

// zero blocks of every plane of both region buffers of the split engines (never overwritten by the DMA)
template <int NS>
__device__ __forceinline__ void zero_blocks(char* __restrict__ rbuf0, int region_bytes, int plane, int zbase) {
  if (threadIdx.x < 2 * NS * 16) {
    const int pl = threadIdx.x >> 4;                             // (buffer, piece) plane index
    *(f4*)(rbuf0 + (size_t)(pl / NS) * region_bytes + (size_t)(pl % NS) * plane + zbase + (threadIdx.x & 15) * 16) = f4{0.f, 0.f, 0.f, 0.f};
  }
}

// ---------------------------------------------------------------- stages B / D
// Grouped k x k convolution as an im2col GEMM.  One workgroup = one conv tile
// (normally a whole period grid, <= 384 pixels) x one branch x NCO output-channel
// tiles.  Per 16-input-channel chunk it stages (a) the tile plus halo, clipped to
// the grid, as [pixel][16 ch] rows of 80 B (16 consecutive pixels hit 16 distinct
// bank quads on ds_read_b128) and (b) that chunk's weight fragments for every tap,
// lane-linear (1 KiB per fragment, conflict-free).  A tap outside the grid is conv
// zero padding: the lane reads a zeroed slot instead (row/column validity bits are
// precomputed per pixel).  The tap loop is software-pipelined: the next tap's LDS
// reads are issued before the current tap's MFMAs.

#define LDS_PX_STRIDE 20  // 16 channels + 4 pad dwords
#define CONV_NU 6         // 16-pixel units per wave: 4 waves x 6 x 16 >= FTN_TILE_PX

// One kernel row (fixed dy) of taps for NU units.  KW > 0: the dx loop is fully
// unrolled (tap offsets become ds_read immediates, no per-tap address math);
// KW == 0: runtime kw.  Row validity is folded into the column mask once per row,
// so a tap costs one bit test + one address select per unit.
template <int NCO, int NU, int KW>
__device__ __forceinline__ void conv_row(f4 (&acc)[NCO][CONV_NU], const float* __restrict__ tile,
                                         const float* __restrict__ wrow, const int (&rowaddr)[NU],
                                         const unsigned (&cmv)[NU], int kw, int zoff) {
  const int n = KW > 0 ? KW : kw;
#pragma unroll
  for (int dx = 0; dx < n; ++dx) {
    f4 bf[NU], af[NCO];
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const bool v = ((cmv[u] >> dx) & 1u) != 0u;
      bf[u] = *(const f4*)(tile + (v ? rowaddr[u] + dx * LDS_PX_STRIDE : zoff));
    }
#pragma unroll
    for (int o = 0; o < NCO; ++o) af[o] = *(const f4*)(wrow + (dx * NCO + o) * 256);
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int o = 0; o < NCO; ++o)
#pragma unroll
        for (int u = 0; u < NU; ++u) acc[o][u] = mfma16(af[o][e], bf[u][e], acc[o][u]);
  }
}

template <int NCO, int NU>
__device__ __forceinline__ void conv_taps(f4 (&acc)[NCO][CONV_NU], const float* __restrict__ tile,
                                          const float* __restrict__ wl, const int (&lbase)[CONV_NU],
                                          const unsigned (&rmask)[CONV_NU], const unsigned (&cmask)[CONV_NU],
                                          int kh, int kw, int RW, int zoff, int lane) {
  const int hy = kh >> 1, hx = kw >> 1;
  for (int dy = 0; dy < kh; ++dy) {
    int rowaddr[NU];
    unsigned cmv[NU];
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      rowaddr[u] = lbase[u] + ((dy - hy) * RW - hx) * LDS_PX_STRIDE;
      cmv[u] = ((rmask[u] >> dy) & 1u) ? cmask[u] : 0u;
    }
    const float* __restrict__ wrow = wl + (size_t)dy * kw * NCO * 256 + lane * 4;
    if (kw == 7) conv_row<NCO, NU, 7>(acc, tile, wrow, rowaddr, cmv, kw, zoff);
    else if (kw == 5) conv_row<NCO, NU, 5>(acc, tile, wrow, rowaddr, cmv, kw, zoff);
    else if (kw == 3) conv_row<NCO, NU, 3>(acc, tile, wrow, rowaddr, cmv, kw, zoff);
    else if (kw == 1) conv_row<NCO, NU, 1>(acc, tile, wrow, rowaddr, cmv, kw, zoff);
    else conv_row<NCO, NU, 0>(acc, tile, wrow, rowaddr, cmv, kw, zoff);
  }
}

template <int NCO>
__global__ __launch_bounds__(256) void k_conv(ConvArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const FtnDesc* __restrict__ d = a.desc;
  const size_t wgid = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
  stamp(a.dbg, a.dbg_cap, wgid, 0);
  stamp_realtime(a.dbg, a.dbg_cap, wgid, 6);
  // grid.x = max_groups (one tile per group is the common case); a workgroup walks the
  // data-dependent tile list with that stride, so no workgroup is dispatched empty unless
  // groups merged (interleaved empty workgroups skew the round-robin XCD placement)
  const int tiles_total = d->tiles_per_row;
  for (int bx = blockIdx.x; bx < tiles_total; bx += gridDim.x) {
  if (bx != (int)blockIdx.x) __syncthreads();
  const int b = blockIdx.y;
  const int zb = blockIdx.z / a.nchunk, chunk = blockIdx.z - zb * a.nchunk;
  const int br = a.order[zb];
  const int kh = a.kh[br], kw = a.kw[br];
  const ConvTile t = conv_tile(d, d->n_groups, bx, kh >> 1, kw >> 1);
  float* __restrict__ tile = lds;
  float* __restrict__ wl = lds + a.region_floats;
  const int zoff = a.region_floats - 16;                 // 16 zero floats at the end of the region area
  const size_t nimg = (size_t)a.B * d->g_px_off[t.g] + (size_t)b * t.P;
  const int btL = a.bt_L;
  const float* __restrict__ in = a.in + (btL > 0 ? (size_t)b * btL : nimg) * a.INC + br * a.in_stride_br;
  const float* __restrict__ in_pad = a.in + (size_t)a.B * btL * a.INC + br * a.in_stride_br;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 15, q = lane >> 4;
  const int wrot = (wave + b) & 3;                                 // rotate so co-resident workgroups balance the SIMDs
  const int nu = t.nunits > wrot ? (t.nunits - wrot + 3) >> 2 : 0;   // units of this wave: wrot, wrot+4, ...
  const int nco_tot = a.cout >> 4, co0 = chunk * NCO;
  const int ncc = a.cin >> 4, ntaps = kh * kw;

  int lbase[CONV_NU], oidx[CONV_NU];
  unsigned rmask[CONV_NU], cmask[CONV_NU];
  bool pok[CONV_NU];
  const float inv_tw = 1.0f / (float)t.tw;
#pragma unroll
  for (int u = 0; u < CONV_NU; ++u) {
    const ConvPixel px = conv_pixel(t, (wrot + 4 * u) * 16 + j, inv_tw, kh, kw);
    pok[u] = px.ok;
    lbase[u] = ((px.ri - t.R0) * t.RW + (px.ci - t.C0)) * LDS_PX_STRIDE + 4 * q;
    oidx[u] = px.ri * t.p + px.ci;
    rmask[u] = px.rm;
    cmask[u] = px.cm;
  }
  f4 acc[NCO][CONV_NU];
#pragma unroll
  for (int o = 0; o < NCO; ++o) {
    f4 bv = {0.f, 0.f, 0.f, 0.f};
    if (co0 + o < nco_tot) bv = *(const f4*)(a.bias + br * a.out_stride_br + 16 * (co0 + o) + 4 * q);
#pragma unroll
    for (int u = 0; u < CONV_NU; ++u) acc[o][u] = bv;
  }
  if (threadIdx.x < 4) *(f4*)(tile + zoff + 4 * threadIdx.x) = f4{0.f, 0.f, 0.f, 0.f};
  const float* __restrict__ Wb = a.W[br];
  const int nstage = t.RH * t.RW * 4;                    // four 16-byte quarters per region pixel
  const float inv_rw = 1.0f / (float)t.RW;
  for (int cc = 0; cc < ncc; ++cc) {
    if (cc > 0) __syncthreads();
    // weight fragments: LDS-DMA (global_load_lds_dwordx4), one 1-KiB fragment per wave
    // instruction, no VGPR round trip; all pieces of a wave are in flight together and the
    // region loads below join the same queue, so staging costs ~one L2 latency.
    {
      const int wv = __builtin_amdgcn_readfirstlane(wave);
      const int npieces = ntaps * NCO;
      for (int piece = wv; piece < npieces; piece += 4) {
        const int tap = piece / NCO, o = piece - tap * NCO;
        if (co0 + o < nco_tot) {
          __builtin_amdgcn_global_load_lds(
              (const __attribute__((address_space(1))) void*)(Wb + ((size_t)(tap * ncc + cc) * nco_tot + co0 + o) * 256 + lane * 4),
              (__attribute__((address_space(3))) void*)(wl + (size_t)piece * 256), 16, 0, 0);
        } else {
          *(f4*)(wl + (size_t)piece * 256 + lane * 4) = f4{0.f, 0.f, 0.f, 0.f};
        }
      }
    }
    for (int s0 = threadIdx.x; s0 < nstage; s0 += 256 * 6) {
      f4 v[6];
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        const int s = s0 + 256 * k;
        const int qq = s & 3;
        const int tpx = t.grid_px(s >> 2, inv_rw);
        const float* __restrict__ row = conv_pad_row(btL, tpx) ? in_pad : in + (size_t)tpx * a.INC;
        v[k] = s < nstage ? *(const f4*)(row + 16 * cc + 4 * qq) : f4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        const int s = s0 + 256 * k;
        if (s < nstage) *(f4*)(tile + (s >> 2) * LDS_PX_STRIDE + 4 * (s & 3)) = v[k];
      }
    }
    __syncthreads();
    if (cc == 0) stamp(a.dbg, a.dbg_cap, wgid, 1);
    switch (nu) {
      case 6: conv_taps<NCO, 6>(acc, tile, wl, lbase, rmask, cmask, kh, kw, t.RW, zoff, lane); break;
      case 5: conv_taps<NCO, 5>(acc, tile, wl, lbase, rmask, cmask, kh, kw, t.RW, zoff, lane); break;
      case 4: conv_taps<NCO, 4>(acc, tile, wl, lbase, rmask, cmask, kh, kw, t.RW, zoff, lane); break;
      case 3: conv_taps<NCO, 3>(acc, tile, wl, lbase, rmask, cmask, kh, kw, t.RW, zoff, lane); break;
      case 2: conv_taps<NCO, 2>(acc, tile, wl, lbase, rmask, cmask, kh, kw, t.RW, zoff, lane); break;
      case 1: conv_taps<NCO, 1>(acc, tile, wl, lbase, rmask, cmask, kh, kw, t.RW, zoff, lane); break;
      default: break;
    }
  }
  stamp(a.dbg, a.dbg_cap, wgid, 2);
  stamp_word(a.dbg, a.dbg_cap, wgid, 4, (unsigned long long)(kh * kw));
  stamp_word(a.dbg, a.dbg_cap, wgid, 5, __builtin_amdgcn_s_getreg(((4 - 1) << 11) | (0 << 6) | 20));  // XCC_ID
  float* __restrict__ out = a.out + nimg * a.OUTC + br * a.out_stride_br;
#pragma unroll
  for (int o = 0; o < NCO; ++o) {
    if (co0 + o < nco_tot) {
#pragma unroll
      for (int u = 0; u < CONV_NU; ++u)
        if (u < nu && pok[u]) *(f4*)(out + (size_t)oidx[u] * a.OUTC + 16 * (co0 + o) + 4 * q) = acc[o][u];
    }
  }
  stamp(a.dbg, a.dbg_cap, wgid, 3);
  stamp_realtime(a.dbg, a.dbg_cap, wgid, 7);
  }  // tile loop
}

// ---------------------------------------------------------------- stages B / D, bf16x3 engine
// Same convolution on the bf16 matrix pipe with fp32-equivalent accuracy: activations arrive
// as three bf16 pieces per value (P3 layout, written by the producing stage), weights are
// pre-split on the host, and every K=32 slab (= two taps x 16 input channels) is six
// v_mfma_f32_16x16x32_bf16 (hi*lo, lo*hi, mid*mid, hi*mid, mid*hi, hi*hi) into one fp32
// accumulator: 96 cycles instead of 256 for the same contraction in fp32 MFMA.
// One 512-thread workgroup (two waves per SIMD) owns one tile x branch and walks `bpw`
// batch rows: the weight fragments are staged once by LDS-DMA, the tile regions are
// double-buffered (row i+1 is requested before row i is computed), so neither is on the
// critical path.  NS = 1 drops the mid/lo pieces (plain bf16, BASELINE configs[2]).

#define CBF_NU 3          // 16-pixel units per wave: 8 waves x 3 x 16 >= FTN_TILE_PX
// LDS image of a staged region: one PLANE per piece, 32 bytes per pixel = [channels 0-7][channels 8-15] of that
// piece.  A ds_read_b128 is served in four groups of 16 lanes - {0-3,12-15,20-27}, {4-11,16-19,28-31} and the
// same + 32 (MI355X_MICROARCH.md, LDS) - and a lane (j = lane & 15, qa = lane >> 4) reads pixel j's half qa & 1:
// with a 32-byte pixel stride the eight half-0 lanes of a group fall on the even 16-byte bank quads and its eight
// half-1 lanes on the odd ones, all distinct, for every tap offset (a constant shift).  Round 1's pixel-major
// image (96 B of pieces + 16 B pad per pixel) put seven of those sixteen lanes on a shared quad.
#define CBF_PX_BYTES 32

template <int NCO, int NS>
__global__ __launch_bounds__(512) void k_conv_bf(ConvBfArgs a) {
  extern __shared__ __attribute__((aligned(16))) char ldsb[];
  constexpr int NWP = PxFmt<NS>::NW;                          // weight pieces
  constexpr int PXE = PxFmt<NS>::ELEMS;                       // 16-bit elements per pixel and 16-channel group in memory
  const FtnDesc* __restrict__ d = a.desc;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 15, qa = lane >> 4;
  bool range_bad = false;                                       // f16x2: an output left the fp16 range
  const int wv = __builtin_amdgcn_readfirstlane(wave);
  const int zb = blockIdx.z / a.nchunk, chunk = blockIdx.z - zb * a.nchunk;
  const int br = a.order[zb];
  const int kh = a.kh[br], kw = a.kw[br], hy = kh >> 1, hx = kw >> 1, ntaps = kh * kw;
  const int S = (ntaps + 1) >> 1;
  const int nco_tot = a.cout >> 4, co0 = chunk * NCO, ncc = a.cin >> 4;
  char* __restrict__ wl = ldsb;
  char* __restrict__ rbuf0 = ldsb + a.wbytes;
  const int plane = a.plane_bytes;
  const int zbase = plane - 256;                             // 256-byte zero block at the end of every plane (256-aligned)
  const int b_begin = blockIdx.y * a.bpw, b_end = min(a.B, b_begin + a.bpw);
  const int G = d->n_groups, tiles_total = d->tiles_per_row;
  zero_blocks<NS>(rbuf0, a.region_bytes, plane, zbase);
  const size_t wgid = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
  stamp(a.dbg, a.dbg_cap, wgid, 0);
  stamp_realtime(a.dbg, a.dbg_cap, wgid, 6);
  stamp_word(a.dbg, a.dbg_cap, wgid, 4, (unsigned long long)ntaps);
  stamp_word(a.dbg, a.dbg_cap, wgid, 5, 0);

  for (int bx = blockIdx.x; bx < tiles_total; bx += gridDim.x) {
    const ConvTile t = conv_tile(d, G, bx, hy, hx);
    const int in_groups = a.INC >> 4;
    const float inv_tw = 1.0f / (float)t.tw, inv_rw = 1.0f / (float)t.RW;
    const int nchunks16 = t.RH * t.RW * 2;                 // 16-byte chunks of one plane (two per pixel)
    const int ppp = (nchunks16 + 63) >> 6;                 // 1-KiB DMA instructions per plane

    // region of batch row b, channel group cc -> buffer `buf`: every lane fetches the 16 bytes (pixel, piece,
    // channel half) that belong at its linear LDS position, so the fold (:1041-1046), the clipped halo and the
    // plane split all happen in the DMA's source addresses
    const int btL = a.bt_L;
    auto dma_region = [&](int b, int cc, int buf) {
      const __bf16* __restrict__ src = a.in + (btL > 0 ? (size_t)b * btL : (size_t)a.B * d->g_px_off[t.g] + (size_t)b * t.P) * in_groups * PXE +
                                       (size_t)(br * a.in_stride_br + cc) * PXE;
      const __bf16* __restrict__ src_pad = a.in + (size_t)a.B * btL * in_groups * PXE + (size_t)(br * a.in_stride_br + cc) * PXE;
      for (int pc = wv; pc < NS * ppp; pc += 8) {
        const int pz = pc / ppp, pi = pc - pz * ppp;
        int ci = pi * 64 + lane;
        if (ci >= nchunks16) ci = nchunks16 - 1;             // tail lanes re-read the last chunk (lands in the plane's slack)
        const int half = ci & 1;
        const int tpx = t.grid_px(ci >> 1, inv_rw);
        const __bf16* __restrict__ row = conv_pad_row(btL, tpx) ? src_pad : src + (size_t)tpx * in_groups * PXE;
        __builtin_amdgcn_global_load_lds(
            (const __attribute__((address_space(1))) void*)(row + pz * 16 + half * 8),
            (__attribute__((address_space(3))) void*)(rbuf0 + (size_t)buf * a.region_bytes + (size_t)pz * plane + (size_t)pi * 1024), 16, 0, 0);
      }
    };
    // weight fragments of slabs [g0, g1) of channel chunk cc -> LDS slots [o][slab - g0][piece]
    const int SG = a.sgroup < S ? a.sgroup : S;               // slabs resident at a time
    auto dma_weights = [&](int cc, int g0, int g1) {
      const int nfr = (g1 - g0) * 3;                          // 1-KiB fragments per output tile
      for (int o = 0; o < NCO; ++o) {
        if (co0 + o < nco_tot) {
          const __bf16* __restrict__ src = a.W[br] + ((size_t)(cc * nco_tot + co0 + o) * S + g0) * 3 * 512;
          for (int f = wv; f < nfr; f += 8)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + (size_t)f * 512 + lane * 8),
                                             (__attribute__((address_space(3))) void*)(wl + ((size_t)o * SG * 3 + f) * 1024), 16, 0, 0);
        } else {
          for (int f = wv; f < nfr; f += 8) *(f4*)(wl + ((size_t)o * SG * 3 + f) * 1024 + lane * 16) = f4{0.f, 0.f, 0.f, 0.f};
        }
      }
    };
    const bool resident = ncc == 1 && SG == S;                // one staging per tile serves every batch row

    // per-lane pixel bookkeeping, once per tile (rotated by the workgroup's batch chunk so the
    // 3-unit waves spread over the SIMDs)
    const int wrot = (wave + (int)blockIdx.y) & 7;
    const int nu = t.nunits > wrot ? (t.nunits - wrot + 7) >> 3 : 0;
    int lbase[CBF_NU], oidx[CBF_NU];
    unsigned rmask[CBF_NU], cmask[CBF_NU];
    bool pok[CBF_NU];
#pragma unroll
    for (int u = 0; u < CBF_NU; ++u) {
      const ConvPixel px = conv_pixel(t, (wrot + 8 * u) * 16 + j, inv_tw, kh, kw);
      pok[u] = px.ok;
      lbase[u] = ((px.ri - t.R0 - hy) * t.RW + (px.ci - t.C0 - hx)) * CBF_PX_BYTES + (qa & 1) * 16;
      oidx[u] = px.ri * t.p + px.ci;
      rmask[u] = px.rm;
      cmask[u] = px.cm;
    }
    __syncthreads();                                          // previous tile's readers are done
    if (resident) dma_weights(0, 0, S);
    if (b_begin < b_end) dma_region(b_begin, 0, 0);
    int it = 0;                                                // region buffer parity
    for (int b = b_begin; b < b_end; ++b) {
      f4 acc[NCO][CBF_NU];
#pragma unroll
      for (int o = 0; o < NCO; ++o) {
        f4 bv = {0.f, 0.f, 0.f, 0.f};
        if (co0 + o < nco_tot) bv = *(const f4*)(a.bias + br * a.out_stride_br + 16 * (co0 + o) + 4 * qa);
#pragma unroll
        for (int u = 0; u < CBF_NU; ++u) acc[o][u] = bv;
      }
      for (int cc = 0; cc < ncc; ++cc) {
        if (!resident) { __syncthreads(); dma_weights(cc, 0, SG); }
        __syncthreads();                                      // region (b, cc) and weights have landed (vmcnt(0))
        if (b == b_begin && cc == 0) stamp(a.dbg, a.dbg_cap, wgid, 1);
        if (b == b_begin + 1 && cc == 0) stamp(a.dbg, a.dbg_cap, wgid, 2);
        // request the next region while this one is consumed
        {
          int nb = b, ncq = cc + 1;
          if (ncq == ncc) { ncq = 0; nb = b + 1; }
          if (nb < b_end) dma_region(nb, ncq, (it + 1) & 1);
        }
        const char* __restrict__ reg = rbuf0 + (size_t)(it & 1) * a.region_bytes;
        ++it;
        // slabs: lane group qa>>1 == 1 works on the odd tap of the pair.  Two-deep software
        // pipeline with ping-pong register sets: the LDS reads of slab s+1 are issued before
        // the MFMAs of slab s (sched_barrier keeps hipcc from re-serialising them).
        int tl = qa >> 1;
        int dy = tl / kw, dx = tl - dy * kw;
        int sload = 0, g0 = 0, g1 = SG;                       // resident slab group [g0, g1)
        auto load_slab = [&](bf8 (&bp)[CBF_NU][NS], bf8 (&ap)[NCO][NWP]) {
          const bool tapok = tl < ntaps;
          const int toff = (dy * t.RW + dx) * CBF_PX_BYTES;
#pragma unroll
          for (int u = 0; u < CBF_NU; ++u) {
            const bool v = tapok && (((rmask[u] >> dy) & (cmask[u] >> dx) & 1u) != 0u);
            const int t = lbase[u] + toff;
            const char* __restrict__ src = reg + (v ? t : ((t & 0xF0) | zbase));   // its own slot of the zero block: no bank conflict
#pragma unroll
            for (int pz = 0; pz < NS; ++pz) bp[u][pz] = *(const bf8*)(src + (size_t)pz * plane);
          }
          const int sa = (sload < g1 ? sload : g1 - 1) - g0;  // slot inside the resident group
#pragma unroll
          for (int o = 0; o < NCO; ++o)
#pragma unroll
            for (int pz = 0; pz < NWP; ++pz) ap[o][pz] = *(const bf8*)(wl + (((size_t)o * SG + sa) * 3 + pz) * 1024 + lane * 16);
          ++sload; tl += 2; dx += 2;
          if (dx >= kw) { dx -= kw; ++dy; }
          if (dx >= kw) { dx -= kw; ++dy; }
        };
        auto mma_slab = [&](const bf8 (&bp)[CBF_NU][NS], const bf8 (&ap)[NCO][NWP]) {
#pragma unroll
          for (int o = 0; o < NCO; ++o)
#pragma unroll
            for (int u = 0; u < CBF_NU; ++u) acc[o][u] = chain_bf<NS>(ap[o], bp[u], acc[o][u]);
        };
        bf8 bA[CBF_NU][NS], aA[NCO][NWP], bB[CBF_NU][NS], aB[NCO][NWP];
        for (;;) {
          const int ng = g1 - g0;
          load_slab(bA, aA);
          int sl = 0;
          for (; sl + 2 <= ng; sl += 2) {
            load_slab(bB, aB);
            __builtin_amdgcn_sched_barrier(0);
            mma_slab(bA, aA);
            __builtin_amdgcn_sched_barrier(0);
            load_slab(bA, aA);
            __builtin_amdgcn_sched_barrier(0);
            mma_slab(bB, aB);
            __builtin_amdgcn_sched_barrier(0);
          }
          if (sl < ng) mma_slab(bA, aA);
          if (g1 >= S) break;
          // next weight group: every wave is done with the resident fragments, then restage and rewind the
          // tap walk to the group's first slab (the pipeline ran one or two slabs past it)
          g0 = g1;
          g1 = g0 + SG < S ? g0 + SG : S;
          __syncthreads();
          dma_weights(cc, g0, g1);
          __syncthreads();
          sload = g0;
          tl = 2 * g0 + (qa >> 1);
          dy = tl / kw;
          dx = tl - dy * kw;
        }
      }
      // store this batch row's tile
      const size_t nimg = (size_t)a.B * d->g_px_off[t.g] + (size_t)b * t.P;
      const float inv = a.inv[br];
#pragma unroll
      for (int o = 0; o < NCO; ++o) {
        if (co0 + o < nco_tot) {
#pragma unroll
          for (int u = 0; u < CBF_NU; ++u) {
            if (u < nu && pok[u]) {
              const int ch = br * a.out_stride_br + 16 * (co0 + o);
              const f4 v = NS == 2 ? acc[o][u] * inv : acc[o][u];
              if (NS == 2 && a.out_p3) range_bad |= h2_bad4(v);
              if (a.out_p3) store_px<NS == 2 ? 2 : 3>((__bf16*)a.out + ((nimg + oidx[u]) * (a.OUTC >> 4) + (ch >> 4)) * PXE, qa, v);
              else *(f4*)((float*)a.out + (nimg + oidx[u]) * a.OUTC + ch + 4 * qa) = v;
            }
          }
        }
      }
    }
  }
  stamp(a.dbg, a.dbg_cap, wgid, 3);
  stamp_realtime(a.dbg, a.dbg_cap, wgid, 7);
  if (NS == 2) raise_range_flag(a.range_flag, range_bad);
}

// ---------------------------------------------------------------- stages B / D, split engines, fast path
// The same convolution for the common geometry - one 16-channel input group and one output tile per branch
// (mid <= 16), kernel 3x3 / 5x5 / 7x7, all slabs' weight fragments resident in LDS - with the tap walk resolved
// at compile time.  In k_conv_bf every slab costs ~45 VALU instructions per wave (per-lane tap counters, two
// shifts + a compare + a select per pixel unit, a 32-bit multiply for the row offset, address adds per piece)
// for 9 MFMAs, and VALU issue, not the matrix pipe, sets its pace (PMC: 7.3 VALU per MFMA).  Here
//   * the slab loop is fully unrolled over the kernel's taps, so each lane half's (dy, dx) is a constant and
//     its LDS offset (dy*RW + dx)*32 two scalar operations;
//   * the per-pixel tap validity (conv zero padding at the grid border) is one bit per slab in a mask built
//     once per tile: bit s of vmask[u] = tap 2s + (lane half) is inside the grid for this lane's pixel;
//   * the region planes sit CBF_FAST_PLANE bytes apart (a constant), so the second piece is a ds_read offset.
// That leaves ~10 VALU per slab: v_bfe, v_add, v_mad per pixel unit and one select for the tap offset.
// A plane = the region's pixels + a 256-byte block of zeros (one 16-byte slot per LDS bank quad) that taps outside
// the grid are redirected to.  A redirected lane reads the slot of ITS OWN would-be address ((addr & 0xF0) in the
// block), so it keeps the bank quad it would have used and a ds_read_b128 lane group stays conflict-free; with one
// shared zero pixel every mixed group paid a 2-way conflict (PMC: 17 % of this kernel's LDS cycles, and LDS time
// is level with MFMA time here).
#define CBF_FAST_ZBASE (FTN_REGION_PX * CBF_PX_BYTES)
#define CBF_FAST_PLANE (CBF_FAST_ZBASE + 256)

// fragment pieces a slab occupies in LDS: f16x2 keeps A1 and A3 only (A2 is formed by the VALU)
template <int NS> struct CbfW { static constexpr int STR = NS == 2 ? 2 : 3; };

template <int NS, int KH, int KW>
__device__ __forceinline__ void conv_fast_row(f4 (&acc)[CBF_NU], const char* __restrict__ reg, const char* __restrict__ wlane,
                                               const int (&ld)[CBF_NU], const unsigned (&vmask)[CBF_NU],
                                               int RW32, bool half1) {
  constexpr int NWP = PxFmt<NS>::NW;
  constexpr int WSTR = CbfW<NS>::STR;
  constexpr int NT = KH * KW, S = (NT + 1) / 2;
  bf8 bA[CBF_NU][NS], aA[NWP], bB[CBF_NU][NS], aB[NWP];
  auto load_slab = [&](int s, bf8 (&bp)[CBF_NU][NS], bf8 (&ap)[NWP]) {
    // taps 2s (lanes 0-31) and 2s+1 (lanes 32-63); a tap index == NT (odd tap count) is masked off by vmask
    const int t0 = 2 * s, t1 = 2 * s + 1 < NT ? 2 * s + 1 : 2 * s;
    const int c0 = (t0 / KW) * RW32 + (t0 % KW) * CBF_PX_BYTES;
    const int c1 = (t1 / KW) * RW32 + (t1 % KW) * CBF_PX_BYTES;
    const int toff = half1 ? c1 : c0;
    // weights first: the slab's first MFMA needs them, and LDS reads return in issue order
    if constexpr (NS == 2) {
      // A2 = A1 * 2^-11 exactly (an fp16 multiply by a power of two, subnormals included - the packer forms it the
      // same way), so it is not read: LDS reads and MFMA time are level in this kernel (9 : 9 per slab), the VALU
      // is not, and four v_pk_mul_f16 replace one ds_read_b128 of every slab
      ap[0] = *(const bf8*)(wlane + (s * WSTR + 0) * 1024);
      ap[2] = *(const bf8*)(wlane + (s * WSTR + 1) * 1024);
      ap[1] = __builtin_bit_cast(bf8, __builtin_bit_cast(h8, ap[0]) * (_Float16)0.00048828125f);
    } else {
#pragma unroll
      for (int pz = 0; pz < NWP; ++pz) ap[pz] = *(const bf8*)(wlane + (s * WSTR + pz) * 1024);
    }
#pragma unroll
    for (int u = 0; u < CBF_NU; ++u) {
      const int t = ld[u] + toff;
      const bool v = ((vmask[u] >> s) & 1u) != 0u;
      const int addr = v ? t : ((t & 0xF0) | CBF_FAST_ZBASE);     // valid ? pixel + tap : its slot of the zero block
#pragma unroll
      for (int pz = 0; pz < NS; ++pz) bp[u][pz] = *(const bf8*)(reg + addr + pz * CBF_FAST_PLANE);
    }
  };
  auto mma_slab = [&](const bf8 (&bp)[CBF_NU][NS], const bf8 (&ap)[NWP]) {
#pragma unroll
    for (int u = 0; u < CBF_NU; ++u) acc[u] = chain_bf<NS>(ap, bp[u], acc[u]);
  };
  // One scheduling region per slab: the LDS reads of slab s+1 interleaved one-for-one with the MFMAs of slab s
  // (sched_group_barrier), so a read batch is never waited for right after its issue: with the reads fenced off
  // behind a sched_barrier hipcc waited lgkmcnt(0) before every other MFMA group, i.e. half of the LDS latency
  // was exposed (the 4-bit lgkmcnt cannot express "all but the 18 newest").
  auto interleave = [&]() {
    static_assert(CBF_NU == 3, "interleave patterns are written for three pixel units per wave");
    if constexpr (NS == 2) {                                  // 8 reads + 4 v_pk_mul_f16 : 9 MFMAs
#pragma unroll
      for (int k = 0; k < 8; ++k) {                           // MFMA first: the wait in front of it then covers
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);    // only reads issued a whole slab earlier
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
      }
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
    } else if constexpr (NS == 3) {                           // 12 reads : 18 MFMAs
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        __builtin_amdgcn_sched_group_barrier(0x008, 3, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
      }
    } else {                                                  // 4 reads : 3 MFMAs
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
      }
    }
  };
  load_slab(0, bA, aA);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int s = 0; s < S; s += 2) {
    if (s + 1 < S) load_slab(s + 1, bB, aB);
    mma_slab(bA, aA);
    if (s + 1 < S) interleave();
    __builtin_amdgcn_sched_barrier(0);
    if (s + 1 < S) {
      if (s + 2 < S) load_slab(s + 2, bA, aA);
      mma_slab(bB, aB);
      if (s + 2 < S) interleave();
      __builtin_amdgcn_sched_barrier(0);
    }
  }
}

// Launch shape: ONE workgroup per CU, each bound to one branch for its whole life; a branch gets a share of the
// workgroups proportional to its cost (host: ~3.1 k + 0.35 k cycles per K-32 slab and batch row) and a workgroup
// a contiguous range of that branch's (tile, batch row) sequence (ftn_conv_walk.h: equal shares, with a step into the
// next tile charged as rows, so the workgroups that cross a tile boundary are not the last to finish).  The branch's
// weight fragments (75 KB for 7x7) are DMA'd once per workgroup instead of once per 8 rows, and every CU finishes at about the same time; the
// (tile, 8-row chunk, branch) grid of k_conv_bf runs 480 unequal workgroups (49 / 25 / 9 taps) on 256 CUs in
// roughly 1.4 rounds - 92 us for 66 us of work (tools/stamps.py).
// NCI = 16-channel input groups per branch (mid 16: 1; mid 32: 2, late round 3).  With two, a workgroup is bound to a
// (branch, output tile) pair - a "virtual branch" - keeps both input groups' fragment sets in LDS and walks the
// (batch row, input group) sequence through the same two region buffers: the second group's products add into the
// first's accumulators, the row's outputs are stored once.
template <int NS, int NCI>
__global__ __launch_bounds__(512) void k_conv_bf_fast(ConvBfArgs a) {
  extern __shared__ __attribute__((aligned(16))) char ldsb[];
  constexpr int PXE = PxFmt<NS>::ELEMS;
  constexpr int plane = CBF_FAST_PLANE;
  constexpr int WSTR = CbfW<NS>::STR;
  const FtnDesc* __restrict__ d = a.desc;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 15, qa = lane >> 4;
  bool range_bad = false;                                       // f16x2: an output left the fp16 range
  const int wv = __builtin_amdgcn_readfirstlane(wave);
  int vb = 0;
  while (vb + 1 < a.nvb && (int)blockIdx.x >= a.wg_off[vb + 1]) ++vb;
  const int wgi = (int)blockIdx.x - a.wg_off[vb], nwg = a.wg_off[vb + 1] - a.wg_off[vb];
  const int nco = a.cout >> 4, br = vb / nco, cot = vb - br * nco;   // branch, output tile of the branch
  const int G = d->n_groups, tiles_total = d->tiles_per_row;
  // this workgroup's positions of the branch's (tile, batch row) sequence, a tile switch charged as sw rows
  const int sw = a.switch_rows[vb];
  int pos[2];
  ftn_conv_walk(tiles_total, a.B, sw, nwg, wgi, pos);
  const int pos_hi = pos[1];
  const size_t wgid = blockIdx.x;
  stamp(a.dbg, a.dbg_cap, wgid, 0);
  if (pos[0] >= pos_hi) return;
  const int kh = a.kh[br], kw = a.kw[br], hy = kh >> 1, hx = kw >> 1, ntaps = kh * kw;
  const int S = (ntaps + 1) >> 1;
  stamp_realtime(a.dbg, a.dbg_cap, wgid, 6);
  stamp_word(a.dbg, a.dbg_cap, wgid, 4, (unsigned long long)ntaps);
  stamp_word(a.dbg, a.dbg_cap, wgid, 5, ((unsigned long long)ftn_conv_walk_row(a.B, sw, pos[0]) << 32) |   // its rows [lo, hi)
                                        (unsigned)ftn_conv_walk_row(a.B, sw, pos_hi));
  char* __restrict__ wl = ldsb;
  char* __restrict__ rbuf0 = ldsb + (size_t)NCI * S * WSTR * 1024;   // behind THIS (branch, tile)'s weight fragments
  static_assert(CBF_FAST_ZBASE % 256 == 0, "the zero block must start on a 256-byte boundary");
  zero_blocks<NS>(rbuf0, a.region_bytes, plane, CBF_FAST_ZBASE);
  {                                                            // every slab of the branch's one output tile, once
    // f16x2: piece 1 (A2 = A1 * 2^-11) is formed by the VALU in the slab loop, so it is neither fetched nor given
    // room in LDS (packed layout: [cin group][cout tile][slab][3 pieces] x 1 KB; LDS: [cin group][slab][WSTR])
    const int npc = S * WSTR;
#pragma unroll
    for (int gi = 0; gi < NCI; ++gi) {
      const __bf16* __restrict__ src = a.W[br] + (size_t)(gi * nco + cot) * S * 3 * 512;
      for (int g = wv; g < npc; g += 8) {
        const int f = NS == 2 ? (g >> 1) * 3 + (g & 1) * 2 : g;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + (size_t)f * 512 + lane * 8),
                                         (__attribute__((address_space(3))) void*)(wl + (size_t)(gi * npc + g) * 1024), 16, 0, 0);
      }
    }
  }
  const f4 bv = *(const f4*)(a.bias + br * a.out_stride_br + 16 * cot + 4 * qa);
  const float inv = a.inv[br];
  const int in_groups = a.INC >> 4;
  const int btL = a.bt_L;
  const int h1 = qa >> 1;                                     // this lane's tap of every pair
  bool first_tile = true;

  int bx, b_begin, b_end;                                      // tile (of the per-row tile list), then its batch rows
  for (int v = pos[0]; ftn_conv_walk_next(a.B, sw, &v, pos_hi, &bx, &b_begin, &b_end);) {
    const ConvTile t = conv_tile(d, G, bx, hy, hx);
    const float inv_tw = 1.0f / (float)t.tw, inv_rw = 1.0f / (float)t.RW;
    const int nchunks16 = t.RH * t.RW * 2;
    const int ppp = (nchunks16 + 63) >> 6;
    // descriptor values the row loop needs, read once per tile (a load inside the loop is a full round trip on
    // the critical path of every batch row, and its s_waitcnt vmcnt(0) also waits for everything else in flight)
    const size_t img0 = (size_t)a.B * d->g_px_off[t.g];
    // Region DMA: which 16-byte chunk a lane fetches for piece k of this wave depends on the tile only, so its
    // offset (relative to the batch row's first pixel, or to the shared pad row for the live zero pixels t >= L)
    // and its LDS slot are worked out once per tile; a batch row then costs an add, a select and the load per piece
    // (generating the addresses in the row loop was ~65 instructions per piece, most of that loop's fixed cost).
    constexpr int KPMAX = (NS * ((FTN_REGION_PX * 2 + 63) / 64) + 7) / 8;
    int poff[KPMAX], pdst[KPMAX];
    unsigned ppad = 0u;
    const int npc = NS * ppp;
#pragma unroll
    for (int k = 0; k < KPMAX; ++k) {
      const int pc = wv + 8 * k;
      const int pcc = pc < npc ? pc : 0;
      const int pz = pcc / ppp, pi = pcc - pz * ppp;
      int ci = pi * 64 + lane;
      if (ci >= nchunks16) ci = nchunks16 - 1;
      const int half = ci & 1;
      const int tpx = t.grid_px(ci >> 1, inv_rw);
      const bool pad = conv_pad_row(btL, tpx);
      poff[k] = (pad ? 0 : tpx * in_groups * PXE) + pz * 16 + half * 8;
      ppad |= (pad ? 1u : 0u) << k;
      pdst[k] = __builtin_amdgcn_readfirstlane(pz * plane + pi * 1024);
    }
    const __bf16* __restrict__ in_br = a.in + (size_t)(br * a.in_stride_br) * PXE;
    const __bf16* __restrict__ src_pad = in_br + (size_t)a.B * btL * in_groups * PXE;
    const size_t row_stride = (size_t)(btL > 0 ? btL : t.P) * in_groups * PXE;
    const __bf16* __restrict__ src0 = in_br + (btL > 0 ? (size_t)0 : img0 * in_groups * PXE);
    auto dma_region = [&](int b, int gi, int buf) {           // input group gi of batch row b
      const __bf16* __restrict__ src = src0 + (size_t)b * row_stride + gi * PXE;
      char* __restrict__ dstb = rbuf0 + (size_t)buf * a.region_bytes;
#pragma unroll
      for (int k = 0; k < KPMAX; ++k) {
        if (wv + 8 * k < npc) {
          const __bf16* __restrict__ rowp = ((ppad >> k) & 1u) ? src_pad + gi * PXE : src;
          __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(rowp + poff[k]),
                                           (__attribute__((address_space(3))) void*)(dstb + pdst[k]), 16, 0, 0);
        }
      }
    };
    // the tile's first row is requested before the per-lane bookkeeping, so it lands meanwhile (the previous
    // tile's readers must be done with the buffers first)
    if (!first_tile) __syncthreads();
    first_tile = false;
    dma_region(b_begin, 0, 0);
    // per-lane pixel bookkeeping, once per tile.  Tap validity (conv zero padding at the grid border): bit s of
    // vmask[u] = tap 2s + h1 lies inside the grid for this lane's pixel, from a row mask and a column mask and a
    // division-free walk over the taps (a runtime tl / kw per slab and unit cost 20 k cycles of a 7x7 tile's
    // 34 k cycle prologue, tools/stamps.py)
    const int wrot = (wave + b_begin) & 7;
    const int nu = t.nunits > wrot ? (t.nunits - wrot + 7) >> 3 : 0;
    int ld[CBF_NU], oidx[CBF_NU];
    unsigned ooff[CBF_NU];
    unsigned vmask[CBF_NU];
    bool pok[CBF_NU];
#pragma unroll
    for (int u = 0; u < CBF_NU; ++u) {
      const ConvPixel px = conv_pixel(t, (wrot + 8 * u) * 16 + j, inv_tw, kh, kw);
      pok[u] = px.ok;
      ld[u] = ((px.ri - t.R0 - hy) * t.RW + (px.ci - t.C0 - hx)) * CBF_PX_BYTES + (qa & 1) * 16;
      oidx[u] = px.ri * t.p + px.ci;
      {
        const int ch = br * a.out_stride_br + 16 * cot;
        ooff[u] = a.out_p3 ? (unsigned)((oidx[u] * (a.OUTC >> 4) + (ch >> 4)) * PXE)
                           : (unsigned)(oidx[u] * a.OUTC + ch + 4 * qa);
      }
      // bit s = tap 2s + h1 is inside the grid.  Row dy of the kernel (kw odd: its first tap has parity dy) holds the
      // taps of this lane half at dx = par, par + 2, ... with par = (dy ^ h1) & 1, i.e. every other bit of the column
      // mask, compressed, at slab (dy kw + par - h1) / 2: ~70 instructions per pixel unit instead of a 10-instruction
      // step per slab (the 7x7 prologue spent 9 k of its 25 k cycles in that loop; tools/stamps.py)
      const unsigned ce = (px.cm & 1u) | ((px.cm >> 1) & 2u) | ((px.cm >> 2) & 4u) | ((px.cm >> 3) & 8u);
      const unsigned co = ((px.cm >> 1) & 1u) | ((px.cm >> 2) & 2u) | ((px.cm >> 3) & 4u) | ((px.cm >> 4) & 8u);
      unsigned m = 0u;
#pragma unroll
      for (int dy = 0; dy < 7; ++dy) {                         // kh <= 7 here (fast path: 3x3 / 5x5 / 7x7)
        const int par = (dy ^ h1) & 1;
        const unsigned bits = par ? co : ce;
        if (dy < kh && ((px.rm >> dy) & 1u)) m |= bits << ((dy * kw + par - h1) >> 1);
      }
      vmask[u] = m;                                            // (empty for a lane past the tile: its row mask is)
    }
    int it = 0;
    int keep = 0;                                             // output stores issued behind the newest region DMA
    const int nst_row = a.dbg != nullptr ? 99 : nu * (a.out_p3 ? 2 : 1);
    const char* __restrict__ wlane = wl + lane * 16;
    for (int b = b_begin; b < b_end; ++b) {
      f4 acc[CBF_NU];
#pragma unroll
      for (int u = 0; u < CBF_NU; ++u) acc[u] = bv;
      // the (row, input group) items walk the two region buffers in turn; the item behind this one is requested now
      // (rolled: one copy of the unrolled slab loops)
#pragma unroll 1
      for (int gi = 0; gi < NCI; ++gi) {
        barrier_keep_vm(keep);                                // this item (and, the first time, the weights) have landed
        keep = gi == NCI - 1 ? __builtin_amdgcn_readfirstlane(nst_row) : 0;   // stores only follow a row's last group
        if (gi == 0) {
          if (b == b_begin) stamp(a.dbg, a.dbg_cap, wgid, 1);
          if (b == b_begin + 1) stamp(a.dbg, a.dbg_cap, wgid, 2);
        }
        if (gi + 1 < NCI) dma_region(b, gi + 1, (it + 1) & 1);
        else if (b + 1 < b_end) dma_region(b + 1, 0, (it + 1) & 1);
        const char* __restrict__ reg = rbuf0 + (size_t)(it & 1) * a.region_bytes;
        ++it;
        const char* __restrict__ wg_ = wlane + (size_t)gi * S * WSTR * 1024;
        if (kw == 7) conv_fast_row<NS, 7, 7>(acc, reg, wg_, ld, vmask, t.RW * CBF_PX_BYTES, h1 != 0);
        else if (kw == 5) conv_fast_row<NS, 5, 5>(acc, reg, wg_, ld, vmask, t.RW * CBF_PX_BYTES, h1 != 0);
        else conv_fast_row<NS, 3, 3>(acc, reg, wg_, ld, vmask, t.RW * CBF_PX_BYTES, h1 != 0);
      }
      // uniform row base + per-lane offsets fixed for the tile (ooff)
      const size_t nimg = img0 + (size_t)b * t.P;
      if (a.out_p3) {
        __bf16* __restrict__ ob = (__bf16*)a.out + nimg * (size_t)(a.OUTC >> 4) * PXE;
#pragma unroll
        for (int u = 0; u < CBF_NU; ++u)
          if (u < nu && pok[u]) {
            const f4 v = NS == 2 ? acc[u] * inv : acc[u];
            if (NS == 2) range_bad |= h2_bad4(v);
            store_px<NS == 2 ? 2 : 3>(ob + ooff[u], qa, v);
          }
      } else {
        float* __restrict__ ob = (float*)a.out + nimg * (size_t)a.OUTC;
#pragma unroll
        for (int u = 0; u < CBF_NU; ++u)
          if (u < nu && pok[u]) *(f4*)(ob + ooff[u]) = NS == 2 ? acc[u] * inv : acc[u];
      }
    }
  }
  stamp(a.dbg, a.dbg_cap, wgid, 3);
  stamp_realtime(a.dbg, a.dbg_cap, wgid, 7);
  if (NS == 2) raise_range_flag(a.range_flag, range_bad);
}

// ---------------------------------------------------------------- host side
// Worst staged region (pixels) of a kh x kw conv over every valid period of a
// window of length L, with the tile geometry of ftn_tile_geometry.
static int conv_region_px(int L, int kh, int kw) {
  int worst = 1;
  const int hy = kh / 2, hx = kw / 2;
  for (int p = 1; p < L; ++p) {
    int pad = (p - (L % p)) % p, cyc = (L + pad) / p;
    if (cyc < 2) continue;
    int tw, th, ntx, nty;
    ftn_tile_geometry(cyc, p, &tw, &th, &ntx, &nty);
    int rw = tw + 2 * hx; if (rw > p) rw = p;
    int rh = th + 2 * hy; if (rh > cyc) rh = cyc;
    if (rw * rh > worst) worst = rw * rh;
  }
  return worst;
}

// heavy branches first (descending tap count)
static void heavy_first(int nbr, const int* kh, const int* kw, int* order) {
  for (int k = 0; k < nbr; ++k) order[k] = k;
  for (int i = 1; i < nbr; ++i) {
    int v = order[i], jj = i - 1;
    while (jj >= 0 && kh[order[jj]] * kw[order[jj]] < kh[v] * kw[v]) { order[jj + 1] = order[jj]; --jj; }
    order[jj + 1] = v;
  }
}

template <int NCO>
static int launch_conv_t(const ConvArgs& ca, dim3 grid, size_t lds, hipStream_t st) {
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)k_conv<NCO>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) { ftn_set_error("hipFuncSetAttribute(k_conv): %s", hipGetErrorString(e)); return (int)e; }
  }
  hipLaunchKernelGGL(k_conv<NCO>, grid, dim3(256), lds, st, ca);
  FTN_CHECK_LAUNCH();
  return 0;
}

int ftn_launch_conv(ConvArgs& ca, int B, int L, int grid_x, hipStream_t st) {
  const int nco_tot = ca.cout / 16;
  int region_px = 1, max_taps = 1;
  for (int k = 0; k < ca.nbr; ++k) {
    int v = conv_region_px(L, ca.kh[k], ca.kw[k]);
    if (v > region_px) region_px = v;
    if (ca.kh[k] * ca.kw[k] > max_taps) max_taps = ca.kh[k] * ca.kw[k];
    if (ca.kh[k] > 31 || ca.kw[k] > 31) { ftn_set_error("conv kernel %dx%d too large", ca.kh[k], ca.kw[k]); return -1; }
  }
  ca.region_floats = ((region_px * LDS_PX_STRIDE + 16) + 63) & ~63;
  // output-channel tiles per workgroup: as many as keep the weight fragments (taps*NCO KiB) + region in LDS
  int NCO = nco_tot >= 4 ? 4 : (nco_tot >= 2 ? 2 : 1);
  const size_t budget = 96 * 1024;
  while (NCO > 1 && (size_t)ca.region_floats * 4 + (size_t)max_taps * NCO * 1024 > budget) NCO >>= 1;
  const size_t lds = (size_t)ca.region_floats * 4 + (size_t)max_taps * NCO * 1024;
  if (lds > 160 * 1024) { ftn_set_error("conv kernel needs %zu B of LDS (kernel too large)", lds); return -1; }
  ca.nchunk = ftn_cdiv(nco_tot, NCO);
  heavy_first(ca.nbr, ca.kh, ca.kw, ca.order);
  ca.dbg = ftn_stamp_buf(1, &ca.dbg_cap);
  dim3 grid(grid_x, B, ca.nbr * ca.nchunk);
  if (NCO == 4) return launch_conv_t<4>(ca, grid, lds, st);
  if (NCO == 2) return launch_conv_t<2>(ca, grid, lds, st);
  return launch_conv_t<1>(ca, grid, lds, st);
}

ConvBfGeom ftn_conv_bf_geom(int L, int nbr, const int* kh, const int* kw, int cout, int npieces) {
  ConvBfGeom gm = {0, 0, 0, 0, 0, 0, false};
  int region_px = 1, smax = 1;
  // k_conv_bf_fast: mid <= 16 (one input group, one output tile per branch) or, f16x2 only, mid 17..32 (two and two),
  // kernels 3x3 / 5x5 / 7x7
  bool sq357 = cout == 16 || (cout == 32 && npieces == 2);
  for (int k = 0; k < nbr; ++k) {
    if (!(kh[k] == kw[k] && (kh[k] == 3 || kh[k] == 5 || kh[k] == 7))) sq357 = false;
    if (kh[k] > 31 || kw[k] > 31) return gm;
    int v = conv_region_px(L, kh[k], kw[k]);
    if (v > region_px) region_px = v;
    int sl = (kh[k] * kw[k] + 1) / 2;
    if (sl > smax) smax = sl;
  }
  gm.plane_bytes = ((region_px * CBF_PX_BYTES + 1023) & ~1023) + 256;    // whole DMA pieces + the zero block (see CBF_FAST_ZBASE)
  gm.region_bytes = npieces * gm.plane_bytes;
  const int nco_tot = cout / 16;
  if (sq357 && region_px <= FTN_REGION_PX && !g_conv_generic) {
    const int nci = cout / 16, wstr = npieces == 2 ? 2 : 3;       // (the fast path is only taken for cin == cout)
    const size_t need = (size_t)nci * smax * wstr * 1024 + 2 * (size_t)npieces * CBF_FAST_PLANE;
    if (need <= 160 * 1024) {
      gm.fast = true; gm.NCO = 1; gm.sgroup = smax;
      gm.plane_bytes = CBF_FAST_PLANE; gm.region_bytes = npieces * CBF_FAST_PLANE;
      gm.wbytes = nci * smax * wstr * 1024;
      gm.lds = need;
      return gm;
    }
  }
  // Output tiles per workgroup: more tiles share every pixel fragment read.  When all slabs' weights do not fit
  // beside the two region buffers, they are staged in groups of `sgroup` slabs.
  for (int nco = nco_tot >= 4 ? 4 : (nco_tot >= 2 ? 2 : 1); nco >= 1; nco >>= 1) {
    const size_t room = 160 * 1024 - 2 * (size_t)gm.region_bytes;
    int sg = (int)(room / ((size_t)nco * 3 * 1024));
    if (sg > smax) sg = smax;
    if (sg >= smax || (sg >= 8 && nco > 1) || nco == 1) {
      if (sg < 1) return gm;
      const size_t w = (size_t)nco * sg * 3 * 1024;
      gm.NCO = nco; gm.lds = w + 2 * (size_t)gm.region_bytes; gm.wbytes = (int)w; gm.sgroup = sg;
      return gm;
    }
  }
  return gm;
}

template <int NCO, int NS>
static int launch_conv_bf_t(const ConvBfArgs& ca, dim3 grid, size_t lds, hipStream_t st) {
  hipError_t e = hipFuncSetAttribute((const void*)k_conv_bf<NCO, NS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) { ftn_set_error("hipFuncSetAttribute(k_conv_bf): %s", hipGetErrorString(e)); return (int)e; }
  hipLaunchKernelGGL((k_conv_bf<NCO, NS>), grid, dim3(512), lds, st, ca);
  FTN_CHECK_LAUNCH();
  return 0;
}

template <int NS>
static int launch_conv_bf_n(const ConvBfArgs& ca, const ConvBfGeom& gm, dim3 grid, hipStream_t st) {
  if (gm.NCO == 4) return launch_conv_bf_t<4, NS>(ca, grid, gm.lds, st);
  if (gm.NCO == 2) return launch_conv_bf_t<2, NS>(ca, grid, gm.lds, st);
  return launch_conv_bf_t<1, NS>(ca, grid, gm.lds, st);
}

template <int NS, int NCI>
static int launch_conv_bf_fast_t(const ConvBfArgs& ca, const ConvBfGeom& gm, dim3 grid, hipStream_t st) {
  hipError_t e = hipFuncSetAttribute((const void*)k_conv_bf_fast<NS, NCI>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)gm.lds);
  if (e != hipSuccess) { ftn_set_error("hipFuncSetAttribute(k_conv_bf_fast): %s", hipGetErrorString(e)); return (int)e; }
  hipLaunchKernelGGL((k_conv_bf_fast<NS, NCI>), grid, dim3(512), gm.lds, st, ca);
  FTN_CHECK_LAUNCH();
  return 0;
}

static int launch_conv_bf_fast(const ConvBfArgs& ca, const ConvBfGeom& gm, dim3 grid, int nsplit, hipStream_t st) {
  if (ca.cin == 32) return launch_conv_bf_fast_t<2, 2>(ca, gm, grid, st);        // mid 32: f16x2 only (conv_bf_geom)
  if (nsplit == 3) return launch_conv_bf_fast_t<3, 1>(ca, gm, grid, st);
  if (nsplit == 2) return launch_conv_bf_fast_t<2, 1>(ca, gm, grid, st);
  return launch_conv_bf_fast_t<1, 1>(ca, gm, grid, st);
}

int ftn_launch_conv_bf(ConvBfArgs& ca, const ConvBfGeom& gm, int B, int grid_x, int nsplit, hipStream_t st, int rows_est) {
  const int nco_tot = ca.cout / 16;
  ca.nchunk = ftn_cdiv(nco_tot, gm.NCO);
  ca.plane_bytes = gm.plane_bytes;
  ca.region_bytes = gm.region_bytes;
  ca.wbytes = gm.wbytes;
  ca.sgroup = gm.sgroup;
  ca.dbg = ftn_stamp_buf(1, &ca.dbg_cap);
  size_t cap4;                                                  // which & 4 (non-null: the bit is set): stage B only
  if (ca.bt_L <= 0 && ftn_stamp_buf(4, &cap4) != nullptr) ca.dbg = nullptr;
  // batch rows per (persistent) workgroup: as many as still leave ~2 workgroups per CU in the launch - each
  // staging of a tile's weights and pixel bookkeeping is shared by the rows (8 rows: -3 % against 4 at B = 256)
  ca.bpw = 1;
  for (int bp = 8; bp > 1; bp >>= 1)
    if ((long long)grid_x * ftn_cdiv(B, bp) * ca.nbr * ftn_cdiv(nco_tot, gm.NCO) >= 448) { ca.bpw = bp; break; }
  heavy_first(ca.nbr, ca.kh, ca.kw, ca.order);
  dim3 grid(grid_x, ftn_cdiv(B, ca.bpw), ca.nbr * ca.nchunk);
  // gm.fast already says cin == cout == 16, or 32 on f16x2: the plan comes from ftn_conv_bf_geom(.., cout, nsplit), and
  // block.hip, the only caller, fills cin = cout = the plan's mid width for both convs
  if (gm.fast) {
    // virtual branches: (branch, 16-channel output tile); with two input groups a batch row walks two slab loops
    const int nco = ca.cout / 16, nvb = ca.nbr * nco;
    static int ncu = 0;
    if (ncu == 0) {
      int dev = 0; hipDeviceProp_t prop;
      if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) ncu = prop.multiProcessorCount;
      if (ncu < FTN_CONV_MAXVB) ncu = 256;
    }
    int slabs[FTN_CONV_MAXVB], nwg[FTN_CONV_MAXVB];
    for (int v = 0; v < nvb; ++v) slabs[v] = (ca.kh[v / nco] * ca.kw[v / nco] + 1) / 2;
    ftn_conv_split(ncu, nvb, slabs, ca.cin / 16, rows_est, nwg);
    ca.nvb = nvb;
    ca.wg_off[0] = 0;
    for (int k = 0; k < nvb; ++k) ca.wg_off[k + 1] = ca.wg_off[k] + nwg[k];
    // a tile switch in whole rows of the branch (the row cost of ftn_conv_split's model): 2 / 1 / 1 for 3x3 / 5x5 / 7x7
    for (int v = 0; v < nvb; ++v)
      ca.switch_rows[v] = g_conv_walk ? (int)(FTN_CONV_SWITCH_KCYC / (3.17 + 0.281 * slabs[v] * (ca.cin / 16)) + 0.5) : 0;
    return launch_conv_bf_fast(ca, gm, dim3((unsigned)ca.wg_off[nvb]), nsplit, st);
  }
  if (nsplit == 3) return launch_conv_bf_n<3>(ca, gm, grid, st);
  if (nsplit == 2) return launch_conv_bf_n<2>(ca, gm, grid, st);
  return launch_conv_bf_n<1>(ca, gm, grid, st);
}
