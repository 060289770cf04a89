// Stages B / D argument blocks, the split engines' LDS plan and the launch entries of conv.hip (gfx950 only).
#pragma once
#include "ftn_common.h"

struct ConvArgs {
  const float* in;       // [N][INC]
  float* out;            // [N][OUTC]
  const float* W[FTN_MAXBR];   // per branch [taps][ncc][nco][lane][4]
  const float* bias;     // [OUTC] (per branch slice at out_off)
  const FtnDesc* desc;
  int B, INC, OUTC;
  int nbr;
  int cin;               // input channels per branch (multiple of 16)
  int cout;              // output channels per branch (multiple of 16)
  int in_stride_br;      // channel offset between branches on the input  (cin or 0)
  int out_stride_br;     // channel offset between branches on the output (cout)
  int nchunk;            // output-channel chunks per branch = ceil(cout/16 / NCO)
  int region_floats;     // LDS floats reserved for the staged region (+ zero slot)
  int kh[FTN_MAXBR], kw[FTN_MAXBR];
  int order[FTN_MAXBR];  // branches sorted by descending tap count (heavy workgroups first)
  int bt_L;              // > 0: `in` holds one row per window position, [B*L + 1][INC] (row B*L = the zero-input
                         // pad pixel), shared by every period group; grid pixel t of batch row b is row
                         // b*L + t for t < L and the pad row otherwise.  0: `in` is per grid pixel, [N][INC]
  unsigned long long* dbg; size_t dbg_cap;
};

struct ConvBfArgs {
  const __bf16* in;      // P3 / H2 [rows][INC/16][pieces][16]
  void* out;             // fp32 [N][OUTC] or P3 / H2 [N][OUTC/16][pieces][16]
  const __bf16* W[FTN_MAXBR];  // per branch [cc][co][slab][piece][lane][8]
  const float* bias;     // f16x2: prescaled by the branch's weight scale
  const FtnDesc* desc;
  int B, INC, OUTC, out_p3;
  int nbr, cin, cout, in_stride_br, out_stride_br, nchunk;
  int plane_bytes;       // one piece plane of a region buffer (32 B per pixel) incl. its zero pixel at the end
  int region_bytes;      // one region buffer = pieces x plane_bytes
  int wbytes;            // weight fragment bytes in LDS
  int bpw;               // batch rows per workgroup
  int sgroup;            // K=32 slabs whose weight fragments are resident at a time (>= max slabs: all of them)
  int kh[FTN_MAXBR], kw[FTN_MAXBR], order[FTN_MAXBR];
  int bt_L;              // as ConvArgs.bt_L: > 0 = input rows per window position + one pad row
  float inv[FTN_MAXBR];  // f16x2: 2^-s of the branch's prescaled weights (applied to the accumulators)
  int wg_off[2 * FTN_MAXBR + 1];   // k_conv_bf_fast: workgroups [wg_off[v], wg_off[v+1]) serve virtual branch v = branch * (cout / 16) + output tile
  int nvb;               // virtual branches of the fast path: nbr * (cout / 16)
  int switch_rows[2 * FTN_MAXBR];  // k_conv_bf_fast: rows a tile switch is charged as in virtual branch v's walk (ftn_conv_walk.h)
  int* range_flag;       // f16x2 piece output (out_p3): set when an output leaves the fp16 range; may be null
  unsigned long long* dbg; size_t dbg_cap;
};

struct ConvBfGeom { int NCO; size_t lds; int plane_bytes, region_bytes, wbytes, sgroup; bool fast; };

// LDS plan of the split conv engines for window length L (npieces = activation piece planes per region:
// 3 bf16x3, 2 f16x2, 1 plain bf16); NCO = 0 when it does not fit.
ConvBfGeom ftn_conv_bf_geom(int L, int nbr, const int* kh, const int* kw, int cout, int npieces);
// Launch entries of conv.hip; grid_x = the caller's bound on the period groups.  k_conv:
int ftn_launch_conv(ConvArgs& ca, int B, int L, int grid_x, hipStream_t st);
// k_conv_bf, or k_conv_bf_fast when gm.fast; nsplit = activation pieces, rows_est = estimated (tile, batch row) items or 0
int ftn_launch_conv_bf(ConvBfArgs& ca, const ConvBfGeom& gm, int B, int grid_x, int nsplit, hipStream_t st, int rows_est);
