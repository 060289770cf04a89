// S1 + S2 of the period selector on gfx950 (FFTPeriodSelector.forward, reference models/timesnet.py:64-123): the rFFT
// amplitudes of x [B][L][C], their lower median over channels and the batch sum of the medians, no host synchronisation.
//
//   k_dft_table*        twiddle tables, built once per L
//   k_spectrum          DFT-as-GEMM on v_mfma_f32_32x32x2_f32 (twiddles x window), |.|, median  -> med[B][F]
//   k_spectrum_row      the same with the batch row resident in LDS (one workgroup per row)
//   k_spectrum_rowq     row-resident and folded a second time (L % 4 == 0); channel-tiled for d_model > 64,
//   k_median_rows       which leaves the medians to a second launch
//   k_colsum            fixed-order fp64 batch sum                                               -> psum[F]
// spectrum_geom() is the one place that knows which of the three forms fits a shape and what it needs; S3 - S5 follow
// in selector.hip.
#include <math.h>
#include <stdlib.h>
#include "ftn_common.h"
#include "ftn_exchange.h"
#include "ftn_median.h"

// ---------------------------------------------------------------- twiddle table
// cos table [L][FPAD] followed by sin table [L][FPAD]; FPAD = F rounded up to 32,
// entries with f >= F are zero.  Angles are reduced with an exact integer modulo
// and evaluated in fp64, so the fp32 table is correctly rounded.
static inline int fpad_of(int L) { return ((L / 2 + 1) + 31) & ~31; }

// Quarter-fold tables (L % 4 == 0), appended behind the two [L][FPAD] planes: for even bins f = 2m and odd bins
// f = 2m + 1 the twiddles at tau = 0 .. L/4, four planes [QP][FQ]: cos even, sin even, cos odd, sin odd
// (QP = L/4 + 1 rounded up to even, FQ = number of even bins rounded up to 32; zero outside).
static inline int qfold_qp(int L) { return ((L / 4 + 1) + 1) & ~1; }
static inline int qfold_fq(int L) { return (((L / 2 + 1) + 1) / 2 + 31) & ~31; }
static inline bool qfold_ok(int L) { return L >= 8 && (L & 3) == 0; }

extern "C" size_t ftn_dft_table_bytes(int L) {
  if (L < 2) return 0;
  size_t n = (size_t)2 * L * fpad_of(L);
  if (qfold_ok(L)) n += (size_t)4 * qfold_qp(L) * qfold_fq(L);
  return n * sizeof(float);
}

__global__ void k_dft_table(float* __restrict__ tab, int L, int F, int FPAD) {
  const int total = L * FPAD;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
    const int t = e / FPAD, f = e - t * FPAD;
    float c = 0.f, s = 0.f;
    if (f < F) {
      const long long m = ((long long)f * t) % L;
      const double ang = 2.0 * (double)m / (double)L;  // in units of pi
      c = (float)cospi(ang);
      s = (float)sinpi(ang);
    }
    tab[e] = c;
    tab[total + e] = s;
  }
}

__global__ void k_dft_table_q(float* __restrict__ qt, int L, int F, int QP, int FQ) {
  const int total = QP * FQ, Q = L / 4;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < 2 * total; e += gridDim.x * blockDim.x) {
    const int odd = e >= total ? 1 : 0;
    const int r = e - odd * total, t = r / FQ, m = r - t * FQ;
    const int f = 2 * m + odd;
    float c = 0.f, s = 0.f;
    if (f < F && t <= Q) {
      const long long k = ((long long)f * t) % L;
      const double ang = 2.0 * (double)k / (double)L;
      c = (float)cospi(ang);
      s = (float)sinpi(ang);
    }
    qt[(size_t)(2 * odd) * total + r] = c;
    qt[(size_t)(2 * odd + 1) * total + r] = s;
  }
}

extern "C" int ftn_dft_table_init(void* table_dev, int L, void* stream) {
  FTN_CHECK_ARG(table_dev && L >= 2, "ftn_dft_table_init: bad table/L=%d", L);
  const int F = L / 2 + 1, FPAD = fpad_of(L);
  const int total = L * FPAD;
  hipLaunchKernelGGL(k_dft_table, dim3(ftn_cdiv(total, 256) < 1024 ? ftn_cdiv(total, 256) : 1024), dim3(256), 0,
                     (hipStream_t)stream, (float*)table_dev, L, F, FPAD);
  FTN_CHECK_LAUNCH();
  if (qfold_ok(L)) {
    const int QP = qfold_qp(L), FQ = qfold_fq(L);
    hipLaunchKernelGGL(k_dft_table_q, dim3(ftn_cdiv(2 * QP * FQ, 256) < 1024 ? ftn_cdiv(2 * QP * FQ, 256) : 1024), dim3(256), 0,
                       (hipStream_t)stream, (float*)table_dev + (size_t)2 * total, L, F, QP, FQ);
    FTN_CHECK_LAUNCH();
  }
  return 0;
}

// |re + i im| as sqrt(re^2 + im^2) with the raw hardware square root (v_sqrt_f32, <= 1 ulp): four instructions
// instead of the ~40 of hypotf's scaling paths, sixteen times per lane after the DFT loop (2 us of the row kernels'
// 25).  The squares of a DFT amplitude of fp32 data stay far inside the fp32 range (|X| <= L max|x|: 1e7 for
// inputs of 3e4 squares to 1e14); below 1e-19 the square underflows and the amplitude reads 0 - noise bins of a
// constant series, which the selector ranks last either way.  All three kernels use this form, so k_spectrum and
// k_spectrum_row stay bit-identical.
__device__ __forceinline__ float amp2(float re, float im) { return __builtin_amdgcn_sqrtf(fmaf(re, re, im * im)); }

// ---------------------------------------------------------------- S1 + S2
// One workgroup = one batch row b and 32 frequency bins.  Wave w owns channel
// tiles w, w+NW, ... (32 channels each): rows of the MFMA are frequencies
// (A = twiddles, read [t][f] so 32 lanes read 128 contiguous bytes), columns are
// channels (B = x[b][t][c], C fastest -> 128 contiguous bytes per half-wave).
// The amplitude tile goes to LDS and the lower median over channels is taken by the wave network of ftn_median.h up
// to 256 channels, beyond that by rank counting (exact ties broken by channel index, i.e. a stable sort).
__global__ __launch_bounds__(256) void k_spectrum(const float* __restrict__ x, int B, int L, int C,
                                                  const float* __restrict__ tab, int F, int FPAD,
                                                  float* __restrict__ med) {
  extern __shared__ __attribute__((aligned(16))) float amp[];  // [32][CS]
  const int CS = C + 1;
  // Workgroup -> (batch row, 32-bin block).  Workgroups are dealt round-robin over the 8 XCDs (blockIdx % 8),
  // each with its own L2: all bin blocks of one batch row are given to the SAME XCD, back to back, so x[b] is
  // fetched from HBM once and re-read from that L2 (a (bin block, b) grid spread a row's blocks over six
  // XCDs and fetched it six times).  Speed only: any mapping is correct.
  const int nfb = FPAD >> 5;
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  const int b = (slot / nfb) * 8 + xcd;
  if (b >= B) return;
  const int f0 = (slot % nfb) * 32;
  const int nw = blockDim.x >> 6, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int i = lane & 31, h = lane >> 5;
  const float* __restrict__ xb = x + (size_t)b * L * C;
  const float* __restrict__ ctab = tab + f0 + i;
  const float* __restrict__ stab = tab + (size_t)L * FPAD + f0 + i;
  const int nct = (C + 31) >> 5;
  // Real input: X[f] = sum_t x[t] e^{-2 pi i f t / L} folds around t = L/2,
  //   Re X[f] =  sum_{tau=0}^{L/2} ce[tau] cos(2 pi f tau / L),   ce[tau] = x[tau] + x[L - tau]
  //   Im X[f] = -sum_{tau=1}^{(L-1)/2} co[tau] sin(2 pi f tau / L), co[tau] = x[tau] - x[L - tau]
  // (tau = 0 and, for even L, tau = L/2 have no partner: ce = x[tau], co = 0), which halves the fp32 MFMA work
  // of the DFT-as-GEMM - the pipe this kernel is bound by - for two extra VALU ops per sample.
  const int KT = (L >> 1) + 1;                         // folded time steps tau = 0 .. L/2
  for (int ct = wave; ct < nct; ct += nw) {
    const int c = ct * 32 + i;
    const bool cok = c < C;
    const int cc = cok ? c : 0;
    f16v re = {0}, im = {0};
    // 8 k-steps (16 folded samples) per iteration, two-deep software pipeline: the loads of block i+1 are issued
    // before the MFMAs of block i (sched_barrier keeps hipcc from sinking them back next to their uses)
    // one guarded k-step (tau = t + h): used for tau = 0, 1 and for the ragged end around L/2
    auto step_guarded = [&](int t) {
      const int tau = t + h;
      const bool tok = tau < KT;
      const int tt = tok ? tau : 0;
      const bool pair = tok && tt > 0 && 2 * tt < L;          // has a distinct partner L - tau
      const float xv = xb[(size_t)tt * C + cc];
      const float xp = xb[(size_t)(pair ? L - tt : tt) * C + cc];
      const float cv = tok ? ctab[(size_t)tt * FPAD] : 0.f;
      const float sv = tok ? stab[(size_t)tt * FPAD] : 0.f;
      const float e = (tok && cok) ? (pair ? xv + xp : xv) : 0.f;
      const float o = (pair && cok) ? xv - xp : 0.f;
      re = __builtin_amdgcn_mfma_f32_32x32x2f32(cv, e, re, 0, 0, 0);
      im = __builtin_amdgcn_mfma_f32_32x32x2f32(sv, o, im, 0, 0, 0);
    };
    step_guarded(0);
    // interior: every tau in [2, tmid) has a distinct partner.  8 k-steps (16 folded samples) per iteration,
    // two-deep software pipeline with constant-stride pointers (no bounds tests, no per-load multiplies):
    // the loads of block i+1 are issued before the MFMAs of block i
    const int nint = (L - 1) / 2 - 1 >= 2 ? (((L - 1) / 2 + 1 - 2) / 16) : 0;     // whole 16-sample blocks in [2, (L-1)/2]
    const int sT = 2 * FPAD, sX = 2 * C;
    const float* pc = ctab + (size_t)(2 + h) * FPAD;
    const float* ps = stab + (size_t)(2 + h) * FPAD;
    const float* px = xb + (size_t)(2 + h) * C + cc;
    const float* pp = xb + (size_t)(L - 2 - h) * C + cc;
    float ac[8], as[8], be[8], bo[8];
    if (nint > 0) {
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float xv = px[k * sX], xp = pp[-(k * sX)];
        ac[k] = pc[k * sT]; as[k] = ps[k * sT]; be[k] = xv + xp; bo[k] = xv - xp;
      }
      pc += 8 * sT; ps += 8 * sT; px += 8 * sX; pp -= 8 * sX;
      // (complete before the loop is entered: see k_spectrum_rowq)
#pragma unroll
      for (int k = 0; k < 8; ++k) asm volatile("" : "+v"(ac[k]), "+v"(as[k]), "+v"(be[k]), "+v"(bo[k]));
    }
    for (int it = 0; it < nint; ++it) {
      float an[8], sn[8], en[8], on[8];
      const bool more = it + 1 < nint;   // wave-uniform
      if (more) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float xv = px[k * sX], xp = pp[-(k * sX)];
          an[k] = pc[k * sT]; sn[k] = ps[k * sT]; en[k] = xv + xp; on[k] = xv - xp;
        }
        pc += 8 * sT; ps += 8 * sT; px += 8 * sX; pp -= 8 * sX;
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        re = __builtin_amdgcn_mfma_f32_32x32x2f32(ac[k], cok ? be[k] : 0.f, re, 0, 0, 0);
        im = __builtin_amdgcn_mfma_f32_32x32x2f32(as[k], cok ? bo[k] : 0.f, im, 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
      if (more) {
#pragma unroll
        for (int k = 0; k < 8; ++k) { ac[k] = an[k]; as[k] = sn[k]; be[k] = en[k]; bo[k] = on[k]; }
      }
    }
    for (int t = 2 + 16 * nint; t < KT; t += 2) step_guarded(t);
    if (cok) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int fi = (r & 3) + 8 * (r >> 2) + 4 * h;
        amp[fi * CS + c] = amp2(re[r], im[r]);
      }
    }
  }
  __syncthreads();
  const int target = (C - 1) >> 1;  // torch.median == sorted[(C-1)//2]
  if (C <= 64) {                                          // nw = 1 or 2 here: four rows a pass tile the 32 evenly
    for (int fb = wave; fb < 32; fb += 4 * nw) {          // rows fb, fb+nw, fb+2nw, fb+3nw
      float m[4];
      wave_lower_median_rows<1, 4>(amp + fb * CS, (size_t)nw * CS, C, lane, m);
      if (lane == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (f0 + fb + r * nw < F) med[(size_t)b * F + f0 + fb + r * nw] = m[r];
      }
    }
    return;
  }
  for (int fl = wave; fl < 32; fl += nw) {
    if (f0 + fl >= F) break;
    const float* __restrict__ row = amp + fl * CS;
    if (C <= 256) {
      float m[1];
      if (C <= 128) wave_lower_median_rows<2, 1>(row, 0, C, lane, m);
      else wave_lower_median_rows<4, 1>(row, 0, C, lane, m);
      if (lane == 0) med[(size_t)b * F + f0 + fl] = m[0];
    } else {
      // generic: stable rank count; a NaN ranks nowhere, so a row that holds one is NaN (torch.median)
      bool bad = false;
      for (int c = lane; c < C; c += 64) bad |= row[c] != row[c];
      if (__builtin_amdgcn_ballot_w64(bad) != 0) {
        if (lane == 0) med[(size_t)b * F + f0 + fl] = NAN;
        continue;
      }
      for (int c = lane; c < C; c += 64) {
        const float v = row[c];
        int cnt = 0;
        for (int c2 = 0; c2 < C; ++c2) {
          const float v2 = row[c2];
          cnt += (v2 < v || (v2 == v && c2 < c)) ? 1 : 0;
        }
        if (cnt == target) med[(size_t)b * F + f0 + fl] = v;
      }
    }
  }
}

// ---------------------------------------------------------------- the row-resident kernels' shared phases
// One wave's [32 bins] x [32 channels] tile of the DFT over nks k-steps (two folded samples each): twiddles pc / ps
// from global memory (stride sT per k-step), the folded row pe / po from LDS (stride sX, conflict-free ds_read_b32).
// Eight k-steps per iteration, the twiddles of block i+1 in flight behind the MFMAs of block i.  Rows past the fold's
// last sample hold zeros in LDS; the twiddles they meet are read unguarded and are finite, so they add nothing.
__device__ __forceinline__ void row_dft(const float* __restrict__ pc, const float* __restrict__ ps,
                                        const float* __restrict__ pe, const float* __restrict__ po, int sT, int sX,
                                        int nks, f16v& re, f16v& im) {
  re = f16v{0};
  im = f16v{0};
  float ac[8], as[8];
  const int nblk = nks >> 3;
  if (nblk > 0) {
#pragma unroll
    for (int k = 0; k < 8; ++k) { ac[k] = pc[k * sT]; as[k] = ps[k * sT]; }
    // the first block's twiddles are complete before the loop is entered: hipcc's wait-count pass otherwise carries
    // "ac / as may still be in flight" round the back edge and puts an s_waitcnt vmcnt(0) in front of the second MFMA
    // of EVERY iteration - i.e. behind the loads just issued for the next block, which undoes the pipelining
    // (MFMA phase at 55 % of the pipe's rate)
#pragma unroll
    for (int k = 0; k < 8; ++k) asm volatile("" : "+v"(ac[k]), "+v"(as[k]));
  }
  for (int it = 0; it < nblk; ++it) {
    float an[8], sn[8], be[8], bo[8];
    const bool more = it + 1 < nblk;
    if (more) {
#pragma unroll
      for (int k = 0; k < 8; ++k) { an[k] = pc[(8 * (it + 1) + k) * sT]; sn[k] = ps[(8 * (it + 1) + k) * sT]; }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) { be[k] = pe[(8 * it + k) * sX]; bo[k] = po[(8 * it + k) * sX]; }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      re = __builtin_amdgcn_mfma_f32_32x32x2f32(ac[k], be[k], re, 0, 0, 0);
      im = __builtin_amdgcn_mfma_f32_32x32x2f32(as[k], bo[k], im, 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
    if (more) {
#pragma unroll
      for (int k = 0; k < 8; ++k) { ac[k] = an[k]; as[k] = sn[k]; }
    }
  }
  for (int ks = nblk * 8; ks < nks; ++ks) {
    re = __builtin_amdgcn_mfma_f32_32x32x2f32(pc[(size_t)ks * sT], pe[ks * sX], re, 0, 0, 0);
    im = __builtin_amdgcn_mfma_f32_32x32x2f32(ps[(size_t)ks * sT], po[ks * sX], im, 0, 0, 0);
  }
}

// Lower medians of the row's amplitude tile amp [>= F rounded up to 8][CS] in LDS, eight bins per wave pass.
__device__ __forceinline__ void row_medians(const float* __restrict__ amp, int CS, int C, int F, int wave, int nw,
                                            int lane, float* __restrict__ med_b) {
  for (int fb = wave * 8; fb < F; fb += nw * 8) {
    float m[8];
    wave_lower_median_rows<1, 8>(amp + (size_t)fb * CS, (size_t)CS, C, lane, m);
    if (lane == 0) {
#pragma unroll
      for (int r = 0; r < 8; ++r)
        if (fb + r < F) med_b[fb + r] = m[r];
    }
  }
}

// ---------------------------------------------------------------- S1 + S2, one batch row per workgroup
// The same DFT and median with x[b] resident in LDS.  k_spectrum gives every (row, 32-bin block) its own
// workgroup, so each of a row's bin blocks re-reads and re-folds x[b] with two dword loads per lane per k-step
// beside the two twiddle loads: four vector-memory instructions per MFMA pair, as much time on the texture path as
// on the matrix pipe.  Here ONE workgroup owns the row: it folds x[b] once into LDS (ce = x[tau] + x[L - tau],
// co = x[tau] - x[L - tau], float4 loads), wave w takes (bin block w % nfb, channel tile w / nfb) and reads its B
// operands with conflict-free ds_read_b32 - the only global loads left in the loop are the twiddles - and the
// whole [FPAD][C] amplitude tile of the row stays in LDS for the medians.  Same MFMA sequence on the same
// operands as k_spectrum: the result is bit-identical.  Needs (KT + 1) * CP * 8 + FPAD * (C + 1) * 4 bytes of LDS
// and nfb * nct <= 16 waves (L = 336, C = 64: 136 KB, 12 waves = three per SIMD); other shapes keep k_spectrum.
__global__ __launch_bounds__(1024) void k_spectrum_row(const float* __restrict__ x, int B, int L, int C,
                                                       const float* __restrict__ tab, int F, int FPAD,
                                                       float* __restrict__ med) {
  extern __shared__ __attribute__((aligned(16))) float lds_row[];
  const int KT = (L >> 1) + 1;                         // folded time steps tau = 0 .. L/2
  const int KTP = (KT + 1) & ~1;                       // rows incl. the zero row an odd KT's last k-step reads
  const int nct = (C + 31) >> 5, CP = nct * 32, CS = C + 1;
  float* __restrict__ ce = lds_row;                    // [KTP][CP]
  float* __restrict__ co = ce + (size_t)KTP * CP;      // [KTP][CP]
  float* __restrict__ amp = co + (size_t)KTP * CP;     // [FPAD][CS]
  const int b = blockIdx.x;
  const int nfb = FPAD >> 5;
  const int tid = threadIdx.x, nthr = blockDim.x;
  const int wave = tid >> 6, lane = tid & 63;
  const float* __restrict__ xb = x + (size_t)b * L * C;
  // ---- fold the row into LDS (same expressions as k_spectrum's step_guarded: bit-identical operands)
  if ((C & 3) == 0 && (((uintptr_t)x) & 15) == 0) {
    // four float4 pairs in flight per thread: a plain load -> fold -> store loop pays one HBM round trip per pass
    const int c4n = CP >> 2, total = KTP * c4n;
    for (int e0 = tid; e0 < total; e0 += 4 * nthr) {
      f4 xv[4], xp[4];
      int tau[4], c[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = e0 + u * nthr;
        tau[u] = e / c4n; c[u] = (e - tau[u] * c4n) * 4;
        const bool ok = e < total && tau[u] < KT && c[u] < C;
        const bool pair = ok && tau[u] > 0 && 2 * tau[u] < L;
        const f4 z = {0.f, 0.f, 0.f, 0.f};
        xv[u] = ok ? *(const f4*)(xb + (size_t)tau[u] * C + c[u]) : z;
        xp[u] = pair ? *(const f4*)(xb + (size_t)(L - tau[u]) * C + c[u]) : z;
        if (!pair) xp[u] = z;
        tau[u] = pair ? tau[u] : -1 - tau[u];           // sign carries `pair` to the store loop
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = e0 + u * nthr;
        if (e >= total) continue;
        const bool pair = tau[u] >= 0;
        const int t = pair ? tau[u] : -1 - tau[u];
        const f4 z = {0.f, 0.f, 0.f, 0.f};
        // pair: x[tau] + x[L - tau] and x[tau] - x[L - tau]; no partner (tau = 0, L/2) or padding: x[tau] (or 0) and 0
        *(f4*)(ce + (size_t)t * CP + c[u]) = pair ? xv[u] + xp[u] : xv[u];
        *(f4*)(co + (size_t)t * CP + c[u]) = pair ? xv[u] - xp[u] : z;
      }
    }
  } else {
    for (int e = tid; e < KTP * CP; e += nthr) {
      const int tau = e / CP, c = e - tau * CP;
      float ve = 0.f, vo = 0.f;
      if (tau < KT && c < C) {
        const bool pair = tau > 0 && 2 * tau < L;
        const float xv = xb[(size_t)tau * C + c];
        if (pair) { const float xp = xb[(size_t)(L - tau) * C + c]; ve = xv + xp; vo = xv - xp; }
        else ve = xv;
      }
      ce[e] = ve; co[e] = vo;
    }
  }
  __syncthreads();
  // ---- DFT: wave -> (bin block, channel tile)
  {
    const int i = lane & 31, h = lane >> 5;
    const int fbk = wave % nfb, ct = wave / nfb;
    const int f0 = fbk * 32;
    const int c = ct * 32 + i;
    const float* __restrict__ pc = tab + f0 + i + (size_t)h * FPAD;
    const float* __restrict__ ps = tab + (size_t)L * FPAD + f0 + i + (size_t)h * FPAD;
    const float* __restrict__ pe = ce + (size_t)h * CP + c;
    const float* __restrict__ po = co + (size_t)h * CP + c;
    const int sT = 2 * FPAD, sX = 2 * CP;
    // twiddle rows tau >= KT of an odd-KT last step meet zero operands; they are inside the table (KT < L for L >= 3)
    f16v re, im;
    row_dft(pc, ps, pe, po, sT, sX, KTP >> 1, re, im);   // k-steps of two folded samples each
    if (c < C) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int fi = (r & 3) + 8 * (r >> 2) + 4 * h;
        amp[(size_t)(f0 + fi) * CS + c] = amp2(re[r], im[r]);
      }
    }
  }
  __syncthreads();
  // ---- lower median over channels (amp has FPAD rows)
  row_medians(amp, CS, C, F, wave, nthr >> 6, lane, med + (size_t)b * F);
}

// ---------------------------------------------------------------- S1 + S2, row-resident, folded twice (L % 4 == 0)
// With H = L/2 and theta = 2 pi f tau / L:  cos(2 pi f (H - tau) / L) = (-1)^f cos(theta) and
// sin(2 pi f (H - tau) / L) = -(-1)^f sin(theta), so the half-folded sums of k_spectrum_row fold once more around
// tau = L/4, separately for even and odd bins:
//   even f:  Re = sum_{tau<=Q} ee[tau] cos,  ee = ce[tau] + ce[H - tau]      Im = sum eo[tau] sin,  eo = co[tau] - co[H - tau]
//   odd  f:  Re = sum_{tau< Q} oe[tau] cos,  oe = ce[tau] - ce[H - tau]      Im = sum oo[tau] sin,  oo = co[tau] + co[H - tau]
// (Q = L/4; at tau = Q: ee = ce[Q], oo = co[Q], eo = oe = 0 - the twiddles there vanish for that parity.)
// Half the fp32 MFMAs of k_spectrum_row - the pipe that kernel is bound by - for two more adds per sample.  A
// wave takes (parity, 32-bin block of that parity, channel tile).  Not bit-identical to the other two kernels
// (the four-term sums round differently, at the 1e-7 level); ranks of a sharded batch all take the same path.
// Channel-tiled form (amp_g != nullptr; d_model > 64, where four fold planes of the whole row no longer fit LDS):
// workgroup (b, blockIdx.y) folds and transforms channels [ctile * blockIdx.y, + ctile) only and writes its
// amplitudes to amp_g [B][F][Ctot]; the medians over all channels are then taken by k_median_rows.
__global__ __launch_bounds__(1024) void k_spectrum_rowq(const float* __restrict__ x, int B, int L, int Ctot,
                                                        const float* __restrict__ qtab, int F, int QP, int FQ,
                                                        int amp_rows, float* __restrict__ med, int ctile,
                                                        float* __restrict__ amp_g) {
  extern __shared__ __attribute__((aligned(16))) float lds_row[];
  const int H = L >> 1, Q = L >> 2;
  // (fused form: gridDim.x = B; tiled form: gridDim = (tiles, B), a row's tiles dispatched together so that what is in
  // flight at any time covers whole rows of x, i.e. every memory channel)
  const int tiled = amp_g != nullptr ? 1 : 0;
  const int c_base = tiled ? (int)blockIdx.x * ctile : 0;
  const int C = Ctot - c_base < ctile ? Ctot - c_base : ctile;      // channels of this workgroup
  const int nct = (C + 31) >> 5, CP = nct * 32, CS = C + 1;
  const size_t plane = (size_t)QP * CP;
  float* __restrict__ fold = lds_row;                  // [4][QP][CP]: ee, eo, oe, oo
  float* __restrict__ amp = lds_row + 4 * plane;       // [amp_rows][CS]
  const int b = tiled ? blockIdx.y : blockIdx.x;
  const int tid = threadIdx.x, nthr = blockDim.x;
  const int wave = tid >> 6, lane = tid & 63;
  const float* __restrict__ xb = x + (size_t)b * L * Ctot + c_base;
  {
    const bool vec = (Ctot & 3) == 0 && (((uintptr_t)x) & 15) == 0;
    const int cw = vec ? 4 : 1, cn = CP / cw, total = QP * cn;
    for (int e0 = tid; e0 < total; e0 += 2 * nthr) {
      f4 x0[2], x1[2], x2[2], x3[2];                   // x[tau], x[L - tau], x[H - tau], x[H + tau]
      int tau[2], c[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int e = e0 + u * nthr;
        tau[u] = e / cn; c[u] = (e - tau[u] * cn) * cw;
        const bool ok = e < total && tau[u] <= Q && c[u] < C;
        const f4 z = {0.f, 0.f, 0.f, 0.f};
        x0[u] = x1[u] = x2[u] = x3[u] = z;
        if (ok) {
          const int t = tau[u];
          if (vec) {
            x0[u] = *(const f4*)(xb + (size_t)t * Ctot + c[u]);
            if (t > 0) x1[u] = *(const f4*)(xb + (size_t)(L - t) * Ctot + c[u]);
            if (t < Q) { x2[u] = *(const f4*)(xb + (size_t)(H - t) * Ctot + c[u]); if (t > 0) x3[u] = *(const f4*)(xb + (size_t)(H + t) * Ctot + c[u]); }
          } else {
            x0[u].x = xb[(size_t)t * Ctot + c[u]];
            if (t > 0) x1[u].x = xb[(size_t)(L - t) * Ctot + c[u]];
            if (t < Q) { x2[u].x = xb[(size_t)(H - t) * Ctot + c[u]]; if (t > 0) x3[u].x = xb[(size_t)(H + t) * Ctot + c[u]]; }
          }
        }
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int e = e0 + u * nthr;
        if (e >= total) continue;
        const int t = tau[u];
        // ce[t] = x[t] + x[L-t] (t = 0: x[0]),  co[t] = x[t] - x[L-t] (t = 0: 0);  partner H - t: x[H-t] +- x[H+t]
        // (t = 0: ce[H] = x[H], co[H] = 0; t = Q has no partner)
        const f4 ce = x0[u] + x1[u];
        const f4 co = t > 0 ? x0[u] - x1[u] : f4{0.f, 0.f, 0.f, 0.f};
        const f4 pe = x2[u] + x3[u];
        const f4 po = (t > 0 && t < Q) ? x2[u] - x3[u] : f4{0.f, 0.f, 0.f, 0.f};
        f4 ee = ce + pe, eo = co - po, oe = ce - pe, oo = co + po;
        if (t >= Q) { eo = f4{0.f, 0.f, 0.f, 0.f}; oe = f4{0.f, 0.f, 0.f, 0.f}; }
        if (t > Q) { ee = f4{0.f, 0.f, 0.f, 0.f}; oo = f4{0.f, 0.f, 0.f, 0.f}; }
        float* dst = fold + (size_t)t * CP + c[u];
        if (vec) {
          *(f4*)(dst) = ee; *(f4*)(dst + plane) = eo; *(f4*)(dst + 2 * plane) = oe; *(f4*)(dst + 3 * plane) = oo;
        } else {
          dst[0] = ee.x; dst[plane] = eo.x; dst[2 * plane] = oe.x; dst[3 * plane] = oo.x;
        }
      }
    }
  }
  __syncthreads();
  {
    const int i = lane & 31, h = lane >> 5;
    const int nfq = FQ >> 5;                           // 32-bin blocks per parity
    const int blk = wave % (2 * nfq), ct = wave / (2 * nfq);
    const int odd = blk >= nfq ? 1 : 0, m0 = (blk - odd * nfq) * 32;
    const int c = ct * 32 + i;
    const size_t tplane = (size_t)QP * FQ;
    const float* __restrict__ pc = qtab + (size_t)(2 * odd) * tplane + (size_t)h * FQ + m0 + i;
    const float* __restrict__ ps = pc + tplane;
    const float* __restrict__ pe = fold + (size_t)(2 * odd) * plane + (size_t)h * CP + c;   // ee | oe
    const float* __restrict__ po = fold + (size_t)(odd ? 3 : 1) * plane + (size_t)h * CP + c;   // eo | oo
    const int sT = 2 * FQ, sX = 2 * CP;
    f16v re, im;
    row_dft(pc, ps, pe, po, sT, sX, QP >> 1, re, im);
    if (c < C && amp_g != nullptr) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int f = 2 * (m0 + (r & 3) + 8 * (r >> 2) + 4 * h) + odd;
        if (f < F) amp_g[((size_t)b * F + f) * Ctot + c_base + c] = amp2(re[r], im[r]);
      }
    } else if (c < C) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int fi = (r & 3) + 8 * (r >> 2) + 4 * h;
        amp[(size_t)(2 * (m0 + fi) + odd) * CS + c] = amp2(re[r], im[r]);
      }
    }
  }
  if (amp_g != nullptr) return;
  __syncthreads();
  row_medians(amp, CS, C, F, wave, nthr >> 6, lane, med + (size_t)b * F);   // amp_rows >= F rounded up to 8
}

// Lower median over the channels of amp_g [rows][C], 64 < C <= 128 (the channel-tiled k_spectrum_rowq): four rows
// per wave.
__global__ __launch_bounds__(256) void k_median_rows(const float* __restrict__ amp_g, long long rows, int C,
                                                     float* __restrict__ med) {
  const int lane = threadIdx.x & 63;
  const long long r0 = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 4;
  if (r0 >= rows) return;
  // a ragged last wave re-reads the last row (never written twice: the store below is guarded)
  const long long last = rows - 1;
  const float* __restrict__ base = amp_g + (size_t)r0 * C;
  float m[4];
  if (r0 + 3 <= last) wave_lower_median_rows<2, 4>(base, (size_t)C, C, lane, m);
  else {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float one[1];
      const long long rr = r0 + r <= last ? r0 + r : last;
      wave_lower_median_rows<2, 1>(amp_g + (size_t)rr * C, 0, C, lane, one);
      m[r] = one[0];
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (r0 + r <= last) med[r0 + r] = m[r];
  }
}

// psum[f] = sum_b med[b][f] in fp64, fixed order: 32 row-strided partial sums per column, combined in index
// order (bitwise reproducible; no atomics).
// With an exchange (XchArgs.world > 0) block i also stores its 32 columns into slot `rank` of every rank's exchange
// buffer (peer device memory, mapped through hipIpcOpenMemHandle) and then turns that slot's sequence word i: plain
// stores, a system-scope fence, a system-scope store of the word - the consumer is ftn_finalize.h's bounded wait.
// The call's half, seq & 1, is chosen here: seq is the launch argument (mode 0) or this rank's call counter + 1 (mode 1).
struct XchArgs {
  char* base[FTN_XCHG_MAXWORLD];     // every rank's buffer (half 0)
  size_t half_bytes;
  const unsigned long long* ctr;     // mode 1: this rank's call counter; nullptr in mode 0
  int world, rank, F_cap;
  unsigned long long seq;
};

__global__ __launch_bounds__(1024) void k_colsum(const float* __restrict__ med, int B, int F,
                                                 double* __restrict__ psum, XchArgs xa) {
  __shared__ double part[32][33];
  const int fl = threadIdx.x & 31, bl = threadIdx.x >> 5;
  const int f = blockIdx.x * 32 + fl;
  double s = 0.0;
  if (f < F)
    for (int b = bl; b < B; b += 32) s += (double)med[(size_t)b * F + f];
  part[bl][fl] = s;
  __syncthreads();
  if (bl != 0) return;                                          // wave 0 of the block holds all 32 storing lanes
  const unsigned long long seq = xa.world > 0 ? ftn_xchg_seq(xa.ctr, xa.seq) : 0ull;
  const size_t hoff = (size_t)(seq & 1) * xa.half_bytes;
  if (f < F) {
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < 32; ++k) t += part[k][fl];
    psum[f] = t;
    for (int r = 0; r < xa.world; ++r) ((double*)(xa.base[r] + hoff))[(size_t)xa.rank * xa.F_cap + f] = t;
  }
  if (xa.world > 0) {
    __threadfence_system();
    if (fl == 0)
      for (int r = 0; r < xa.world; ++r)
        __hip_atomic_store((unsigned long long*)(xa.base[r] + hoff + ftn_xchg_flags_off(xa.world, xa.F_cap)) +
                               (size_t)xa.rank * FTN_XCHG_NBLK + blockIdx.x,
                           seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// ---------------------------------------------------------------- geometry and form choice
static const size_t FTN_LDS_LIMIT = 160 * 1024;     // bytes of LDS one workgroup can be given
static const int FTN_MAX_WAVES = 16;                // waves of a 1024-thread workgroup
static const int FTN_GRID_YZ_MAX = 65535;           // gridDim.y / gridDim.z limit

// Everything the three forms need of a shape: what the kernels index by, each form's dynamic LDS and block size, and
// whether it fits.  The choice, the scratch query and the launch all read this one copy, so a form cannot be chosen by
// one rule and launched by another.
struct SpectrumGeom {
  int F, FPAD, nfb, nct;               // bins, bins rounded up to 32, 32-bin blocks, 32-channel tiles
  int KTP;                             // half-folded time steps, rounded up to even
  int QP, FQ, amp_rows;                // quarter fold: time steps, bins per parity, rows of its amplitude tile
  size_t lds_plain, lds_row, lds_q, lds_tile;
  int thr_plain, thr_row, thr_q, thr_tile;
  bool row_fits, q_fits, qtile_fits;
};
static SpectrumGeom spectrum_geom(int B, int L, int C) {
  SpectrumGeom g;
  g.F = L / 2 + 1; g.FPAD = fpad_of(L); g.nfb = g.FPAD / 32; g.nct = (C + 31) / 32;
  g.KTP = (g.F + 1) & ~1;
  g.QP = qfold_qp(L); g.FQ = qfold_fq(L);
  g.amp_rows = ((2 * g.FQ > g.FPAD ? 2 * g.FQ : g.FPAD) + 7) & ~7;
  const size_t tile = (size_t)(C + 1) * sizeof(float);            // one bin's amplitudes, padded against bank conflicts
  const int nfq = g.FQ / 32;
  // k_spectrum: [32][C + 1] amplitudes; one wave per channel tile, four at most
  g.lds_plain = 32 * tile;
  g.thr_plain = 64 * (g.nct < 4 ? g.nct : 4);
  // k_spectrum_row: ce, co [KTP][32 nct] and [FPAD][C + 1] amplitudes; a wave per (bin block, channel tile)
  g.lds_row = (size_t)g.KTP * g.nct * 32 * 2 * sizeof(float) + g.FPAD * tile;
  g.thr_row = 64 * g.nfb * g.nct;
  g.row_fits = C <= 64 && g.nfb * g.nct <= FTN_MAX_WAVES && g.lds_row <= FTN_LDS_LIMIT && L >= 3;
  // k_spectrum_rowq: four fold planes [QP][32 nct] and [amp_rows][C + 1]; a wave per (parity, bin block, channel tile)
  g.lds_q = (size_t)4 * g.QP * g.nct * 32 * sizeof(float) + g.amp_rows * tile;
  g.thr_q = 64 * 2 * nfq * g.nct;
  g.q_fits = qfold_ok(L) && C <= 64 && 2 * nfq * g.nct <= FTN_MAX_WAVES && g.lds_q <= FTN_LDS_LIMIT;
  // channel-tiled k_spectrum_rowq: 64 < C <= 128 (k_median_rows' network), the four fold planes of one 32-channel tile,
  // amplitudes through the caller's scratch; batch rows ride on gridDim.y
  g.lds_tile = (size_t)4 * g.QP * 32 * sizeof(float);
  g.thr_tile = 64 * 2 * nfq;
  // (any B: the launch takes slices of at most FTN_GRID_YZ_MAX rows)
  g.qtile_fits = qfold_ok(L) && C > 64 && C <= 128 && 2 * nfq <= FTN_MAX_WAVES && g.lds_tile <= FTN_LDS_LIMIT;
  return g;
}

extern "C" size_t ftn_period_spectrum_scratch_bytes(int B, int L, int C) {
  if (B < 1 || L < 2 || C < 1 || !spectrum_geom(B, L, C).qtile_fits) return 0;
  return (size_t)B * (L / 2 + 1) * C * sizeof(float);
}

// The form ftn_period_spectrum takes (ftn_period_spectrum_form): 0 k_spectrum, 1 k_spectrum_row, 2 k_spectrum_rowq,
// 3 channel-tiled k_spectrum_rowq + k_median_rows.  Row-resident forms where the folded row and its amplitude tile fit
// LDS and there are rows enough to fill the chip; FTN_SEL_ROW: 0 = k_spectrum, 1 = k_spectrum_row, 2 = k_spectrum_rowq,
// unset = fastest form that fits (k_spectrum and k_spectrum_row are bit-identical, tests compare them).
static int spectrum_form(const SpectrumGeom& g, int B, bool scratch) {
  static const int row_mode = [] { const char* e = getenv("FTN_SEL_ROW"); return e == nullptr ? -1 : atoi(e); }();
  if (scratch && g.qtile_fits && row_mode != 0 && row_mode != 1) return 3;
  if (g.q_fits && (row_mode == 2 || (row_mode < 0 && B >= 64))) return 2;
  if (g.row_fits && (row_mode == 1 || (row_mode < 0 && B >= 64))) return 1;
  return 0;
}

extern "C" int ftn_period_spectrum_form(int B, int L, int C, int x_misalign, int scratch) {
  FTN_CHECK_ARG(B >= 1 && L >= 2 && C >= 1 && x_misalign >= 0 && x_misalign < 16 && x_misalign % 4 == 0,
                "ftn_period_spectrum_form: bad shape B=%d L=%d C=%d misalign=%d", B, L, C, x_misalign);
  const int form = spectrum_form(spectrum_geom(B, L, C), B, scratch != 0);
  // k_spectrum has only scalar loads; the row forms read float4 when C % 4 == 0 and x is 16-byte aligned
  return form + (form != 0 && (C & 3) == 0 && x_misalign == 0 ? 4 : 0);
}

// more dynamic LDS than the 64 KB a kernel gets by default (set per call: the attribute is per device)
static int allow_lds(const void* kernel, size_t bytes, const char* what) {
  hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e != hipSuccess) { ftn_set_error("%s: %s", what, hipGetErrorString(e)); return (int)e; }
  return 0;
}

extern "C" int ftn_period_spectrum(const float* x_dev, int B, int L, int C, const void* table_dev,
                                   float* med_dev, double* psum_dev, void* stream, const FtnExchange* xch,
                                   void* scratch_dev) {
  FTN_CHECK_ARG(x_dev && table_dev && med_dev && psum_dev, "ftn_period_spectrum: null pointer");
  FTN_CHECK_ARG(xch == nullptr || ftn_xch_ok(xch, L / 2 + 1), "ftn_period_spectrum: bad exchange (world / rank / seq / mode / F_cap)");
  FTN_CHECK_ARG(xch == nullptr || ftn_xch_mapped(xch), "ftn_period_spectrum: an exchange slot is not mapped");
  FTN_CHECK_ARG(B >= 1 && L >= 2 && C >= 1, "ftn_period_spectrum: bad shape B=%d L=%d C=%d", B, L, C);
  FTN_CHECK_ARG((long long)(B + 7) * (fpad_of(L) / 32) < 0x7fffffffLL, "ftn_period_spectrum: B=%d too large", B);
  const SpectrumGeom g = spectrum_geom(B, L, C);
  FTN_CHECK_ARG(g.lds_plain <= FTN_LDS_LIMIT, "ftn_period_spectrum: C=%d too large for the LDS amplitude tile", C);
  const hipStream_t st = (hipStream_t)stream;
  const float* tab = (const float*)table_dev;
  const float* qtab = tab + (size_t)2 * L * g.FPAD;
  const int form = spectrum_form(g, B, scratch_dev != nullptr);
  int rc = 0;
  if (form == 3) {
    // d_model > 64: (row, 32-channel tile) workgroups, amplitudes through the caller's scratch, medians in a second launch
    if ((rc = allow_lds((const void*)k_spectrum_rowq, g.lds_tile, "hipFuncSetAttribute(k_spectrum_rowq)")) != 0) return rc;
    // Batch rows ride on gridDim.y, so a batch beyond its limit goes in slices of rows, each with its own part of x, of
    // the scratch and of med: a workgroup sees only its own row, and a median is an exact selection, so every row gets
    // the bits a single launch gives it.
    for (int b0 = 0; b0 < B; b0 += FTN_GRID_YZ_MAX) {
      const int nb = B - b0 < FTN_GRID_YZ_MAX ? B - b0 : FTN_GRID_YZ_MAX;
      float* amp_g = (float*)scratch_dev + (size_t)b0 * g.F * C;
      float* med_s = med_dev + (size_t)b0 * g.F;
      hipLaunchKernelGGL(k_spectrum_rowq, dim3((unsigned)g.nct, (unsigned)nb), dim3(g.thr_tile), g.lds_tile, st,
                         x_dev + (size_t)b0 * L * C, nb, L, C, qtab, g.F, g.QP, g.FQ, 0, med_s, 32, amp_g);
      FTN_CHECK_LAUNCH();
      const long long rows = (long long)nb * g.F;
      hipLaunchKernelGGL(k_median_rows, dim3((unsigned)((rows + 15) / 16)), dim3(256), 0, st, (const float*)amp_g, rows, C, med_s);
      if (b0 + nb < B) FTN_CHECK_LAUNCH();
    }
  } else if (form == 2) {
    if ((rc = allow_lds((const void*)k_spectrum_rowq, g.lds_q, "hipFuncSetAttribute(k_spectrum_rowq)")) != 0) return rc;
    hipLaunchKernelGGL(k_spectrum_rowq, dim3((unsigned)B), dim3(g.thr_q), g.lds_q, st, x_dev, B, L, C, qtab, g.F, g.QP, g.FQ,
                       g.amp_rows, med_dev, C, (float*)nullptr);
  } else if (form == 1) {
    if ((rc = allow_lds((const void*)k_spectrum_row, g.lds_row, "hipFuncSetAttribute(k_spectrum_row)")) != 0) return rc;
    hipLaunchKernelGGL(k_spectrum_row, dim3((unsigned)B), dim3(g.thr_row), g.lds_row, st, x_dev, B, L, C, tab, g.F, g.FPAD,
                       med_dev);
  } else {
    if (g.lds_plain > 64 * 1024 && (rc = allow_lds((const void*)k_spectrum, g.lds_plain, "hipFuncSetAttribute")) != 0) return rc;
    hipLaunchKernelGGL(k_spectrum, dim3((unsigned)(ftn_cdiv(B, 8) * 8 * g.nfb)), dim3(g.thr_plain), g.lds_plain, st, x_dev, B,
                       L, C, tab, g.F, g.FPAD, med_dev);
  }
  FTN_CHECK_LAUNCH();
  XchArgs xa = {};
  if (xch != nullptr) {
    for (int r = 0; r < xch->world; ++r) xa.base[r] = (char*)xch->slots[r];
    xa.half_bytes = ftn_xchg_half_bytes(xch->world, xch->F_cap);
    xa.ctr = ftn_xch_counter(xch);
    xa.world = xch->world; xa.rank = xch->rank; xa.F_cap = xch->F_cap; xa.seq = xch->seq;
  }
  hipLaunchKernelGGL(k_colsum, dim3(ftn_cdiv(g.F, 32)), dim3(1024), 0, st, med_dev, B, g.F, psum_dev, xa);
  FTN_CHECK_LAUNCH();
  return 0;
}
