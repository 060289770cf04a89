// Series groups along an axis that is not the fastest one: x is [outer][S][inner] with inner contiguous, and
// out[o][g][i] = the sum of x[o][s][i] over the members s of group g - the column x[o][.][i] summed by the rules of
// ftn_group_sum word for word (include/flowtimes.h: chunks of 32 members in fp64 left to right from +0.0, the chunk
// sums in ascending order in fp64, one rounding), so the result equals ftn_group_sum on the transposed copy bit for
// bit.  One read of x from HBM, no copy, and no limit on S: the member axis is walked, not staged.
//
// k_group_sum_rows<VEC>: a workgroup walks tiles (o, TI consecutive inner columns), tile = blockIdx.x, + gridDim.x, ..
// Once, it forms the first chunk of every group (cfirst [G + 1], a prefix sum over the device offsets) in LDS.  A
// tile takes the chunks in passes of CP = FTN_GROUP_TILE_BYTES / (8 TI), so TI follows inner alone - a member row's
// TI columns are one contiguous run, all of the row up to 64 columns - however many chunks there are.  Per pass it
//   sums     work items (chunk, column) - VEC: (chunk, quad of columns) - columns fastest along the lanes: an item
//            reads its chunk's <= 32 members from `order`, loads their elements in two batches of RS_BATCH (the loads
//            do not depend on the add chain; 16 quads in flight a lane keep the kernel at 90 VGPRs without scratch) and adds them in fp64; a member slot beyond the chunk's end, or a member
//            outside 0 .. S - 1, loads nothing and adds +0.0 - a sum that starts at +0.0 is never -0.0, so that
//            changes no bit.  The chunk sum goes to csum[chunk of the pass][column], fp64 in LDS: item t writes the
//            8 W bytes at 8 W t, consecutive lanes on consecutive banks;
//   combines after a barrier, one thread per (group, column or quad), columns fastest: the group's chunk sums of this
//            pass in ascending order.  A group that ends in the pass is rounded and stored; the one group that runs
//            past the pass's end leaves its fp64 running sum in carry[pass & 1][column], and the next pass starts
//            that group from there - the same chain of additions, cut at a barrier.  Consecutive lanes read
//            consecutive fp64 words of one csum row (one bank pair each) and store consecutive elements of out.
//            Lanes of different groups in one 32-lane half read rows cfirst[g] TI words apart and can meet on a bank
//            when TI < 32; the combine reads one word per 32 loaded elements, so the rows are left unpadded.
// Neither TI, the passes, the grid, the load width, outer nor inner enters a column's sum.  The device CSR is read
// through ftn_groups.h alone, which clamps what it reads, and a member outside 0 .. S - 1 loads nothing, so a CSR that
// disagrees with the validated host copy cannot address anything outside x, order, out and the workgroup's LDS.
#include "ftn_groups.h"

#define RS_THREADS 1024
#define RS_GRID_MAX 2048
#define RS_BATCH 16

struct GroupRowsArgs {
  const float* x;  float* out;  FtnGroupCsr csr;
  long long inner, outer_stride, member_stride, tiles, work;    // tiles along inner; work = outer tiles
  int S, TI, CP;                                                // TI columns a tile, CP chunks a pass
};

// The form every entry point takes (include/flowtimes.h): the one place the choice is made.
static inline int group_rows_pass(int TI) { return FTN_GROUP_TILE_BYTES / (8 * TI); }
static inline int group_rows_form(long long inner, long long member_stride, long long outer_stride, unsigned misalign,
                                  int C) {
  long long TI = inner < FTN_GROUP_TILE_COLS ? inner : FTN_GROUP_TILE_COLS;
  if (TI >= 4) TI &= ~3LL;
  const bool vec = inner % 4 == 0 && member_stride % 4 == 0 && outer_stride % 4 == 0 && (misalign & 15) == 0;
  const int CP = group_rows_pass((int)TI);
  return (vec ? FTN_SHELL_VEC : 0) | (int)TI << 8 | (C > CP ? (C + CP - 1) / CP : 1) << 16;
}

__device__ __forceinline__ void rs_add(double (&acc)[4], f4 v) {
  acc[0] += (double)v.x; acc[1] += (double)v.y; acc[2] += (double)v.z; acc[3] += (double)v.w;
}
__device__ __forceinline__ void rs_add(double (&acc)[1], float v) { acc[0] += (double)v; }
__device__ __forceinline__ f4 rs_round(const double (&acc)[4]) {
  return f4{(float)acc[0], (float)acc[1], (float)acc[2], (float)acc[3]};
}
__device__ __forceinline__ float rs_round(const double (&acc)[1]) { return (float)acc[0]; }

template <bool VEC>
__global__ __launch_bounds__(RS_THREADS) void k_group_sum_rows(GroupRowsArgs a) {
  using Ld = typename std::conditional<VEC, f4, float>::type;
  constexpr int W = VEC ? 4 : 1;
  extern __shared__ __attribute__((aligned(16))) unsigned char rs_lds[];
  double* csum = (double*)rs_lds;                               // [CP][TI]
  double* carry = csum + (size_t)a.CP * a.TI;                   // [2][TI]
  int* cfirst = (int*)(carry + 2 * a.TI);                       // [G + 1]
  int* part = cfirst + a.csr.G + 1;                             // [RS_THREADS]
  const int tid = threadIdx.x, G = a.csr.G, C = a.csr.C;
  ftn_csr_first_wg(a.csr, RS_THREADS, part, cfirst);

  const int QI = a.TI / W;                                      // VEC: inner % 4 == 0, so TI % 4 == 0
  for (long long work = blockIdx.x; work < a.work; work += gridDim.x) {
    const long long o = work / a.tiles, i0 = (work - o * a.tiles) * a.TI;
    const int live = a.inner - i0 < a.TI ? (int)(a.inner - i0) : a.TI;      // VEC: live % 4 == 0
    const int QL = live / W;
    const float* xb = a.x + o * a.outer_stride + i0;
    float* ob = a.out + o * G * a.inner + i0;
    int pass = 0;
    for (int c0 = 0; c0 < C || pass == 0; c0 += a.CP, ++pass) {             // with no chunk at all: one pass of +0
      const int c1 = c0 + a.CP < C ? c0 + a.CP : C;
      for (int it = tid; it < (c1 - c0) * QI; it += RS_THREADS) {
        const int cl = it / QI, col = (it - cl * QI) * W;
        if (col >= live) continue;
        const FtnGroupChunk k = ftn_csr_chunk(a.csr, cfirst, c0 + cl);
        double acc[W];
#pragma unroll
        for (int w = 0; w < W; ++w) acc[w] = 0.0;
#pragma unroll 1
        for (int j0 = 0; j0 < FTN_GROUP_CHUNK; j0 += RS_BATCH) {
          Ld v[RS_BATCH];
#pragma unroll
          for (int j = 0; j < RS_BATCH; ++j) {
            const int s = j0 + j < k.len ? a.csr.order[k.start + j0 + j] : -1;
            v[j] = Ld(0.f);
            if ((unsigned)s < (unsigned)a.S) v[j] = *(const Ld*)(xb + (long long)s * a.member_stride + col);
          }
#pragma unroll
          for (int j = 0; j < RS_BATCH; ++j) rs_add(acc, v[j]);
        }
#pragma unroll
        for (int w = 0; w < W; ++w) csum[cl * a.TI + col + w] = acc[w];
      }
      __syncthreads();
      const double* cin = carry + ((pass & 1) ^ 1) * a.TI;
      double* cout = carry + (pass & 1) * a.TI;
      for (int w = tid; w < G * QL; w += RS_THREADS) {
        const int g = w / QL, col = (w - g * QL) * W;
        const int s = cfirst[g], e = cfirst[g + 1];
        const int k0 = s > c0 ? s : c0, k1 = s == e ? k0 : e < c1 ? e : c1;
        if (s == e ? pass != 0 : k0 >= k1) continue;            // an empty group: +0, stored by the first pass
        double acc[W];
#pragma unroll
        for (int i = 0; i < W; ++i) acc[i] = s < k0 ? cin[col + i] : 0.0;   // it began in an earlier pass
        for (int k = k0; k < k1; ++k) {
#pragma unroll
          for (int i = 0; i < W; ++i) acc[i] += csum[(k - c0) * a.TI + col + i];
        }
        if (s < e && k1 < e) {                                  // at most one group runs past the pass's end
#pragma unroll
          for (int i = 0; i < W; ++i) cout[col + i] = acc[i];
        } else {
          *(Ld*)(ob + g * a.inner + col) = rs_round(acc);
        }
      }
      __syncthreads();                                          // the next pass writes csum
    }
  }
}

static int group_rows_form_check(const char* who, long long inner, long long member_stride, long long outer_stride,
                                 int n_chunks) {
  FTN_CHECK_ARG(inner >= 1, "%s: inner=%lld is not positive", who, inner);
  FTN_CHECK_ARG(member_stride >= inner, "%s: member stride %lld is below inner=%lld", who, member_stride, inner);
  FTN_CHECK_ARG(outer_stride >= 0, "%s: outer stride %lld is negative", who, outer_stride);
  FTN_CHECK_ARG(n_chunks >= 0 && n_chunks <= FTN_GROUP_CHUNKS_MAX, "%s: %d chunks are outside 0..%d", who, n_chunks,
                FTN_GROUP_CHUNKS_MAX);
  return 0;
}

extern "C" int ftn_group_sum_rows_form(long long inner, long long member_stride, long long outer_stride,
                                       int misalign_or, int n_chunks) {
  if (group_rows_form_check("ftn_group_sum_rows_form", inner, member_stride, outer_stride, n_chunks) < 0) return -1;
  FTN_CHECK_ARG(misalign_ok(misalign_or), "ftn_group_sum_rows_form: misalign=%d", misalign_or);
  return group_rows_form(inner, member_stride, outer_stride, (unsigned)misalign_or, n_chunks);
}

extern "C" int ftn_group_sum_rows(const float* x_dev, long long outer, int S, long long inner, long long outer_stride,
                                  long long member_stride, const int* order_dev, const int* offsets_dev,
                                  const int* offsets_host, int G, int M, float* out_dev, void* stream) {
  const char* who = "ftn_group_sum_rows";
  int chunks = 0;
  if (group_csr_check(who, x_dev, out_dev, order_dev, offsets_dev, offsets_host, G, M, &chunks) < 0) return -1;
  FTN_CHECK_ARG(S >= 1, "%s: S=%d is not positive", who, S);
  FTN_CHECK_ARG(outer >= 1, "%s: outer=%lld is not positive", who, outer);
  if (outer == 1) outer_stride = 0;                             // one slab: its stride addresses nothing
  if (group_rows_form_check(who, inner, member_stride, outer_stride, chunks) < 0) return -1;
  long long span = 0, reach = 0, cells = 0;                     // every product in 64 bits
  FTN_CHECK_ARG(!__builtin_mul_overflow((long long)S, member_stride, &span),
                "%s: S=%d members %lld apart pass 64 bits", who, S, member_stride);
  FTN_CHECK_ARG(outer == 1 || outer_stride >= span, "%s: outer stride %lld is below S member_stride = %lld", who,
                outer_stride, span);
  FTN_CHECK_ARG(!__builtin_mul_overflow(outer, outer_stride, &reach) && reach <= (1LL << 61),
                "%s: outer=%lld slabs %lld apart pass 64 bits", who, outer, outer_stride);
  FTN_CHECK_ARG(!__builtin_mul_overflow(outer, (long long)G, &cells) && !__builtin_mul_overflow(cells, inner, &cells) &&
                    cells <= (1LL << 61),
                "%s: outer=%lld G=%d inner=%lld pass 64 bits", who, outer, G, inner);
  const unsigned misalign = (unsigned)(((uintptr_t)x_dev | (uintptr_t)out_dev) & 15);
  const int form = group_rows_form(inner, member_stride, outer_stride, misalign, chunks);
  GroupRowsArgs a = {};
  a.x = x_dev; a.out = out_dev; a.csr = {order_dev, offsets_dev, G, M, chunks};
  a.inner = inner; a.outer_stride = outer_stride; a.member_stride = member_stride;
  a.S = S; a.TI = (form >> 8) & 255;
  a.tiles = (inner + a.TI - 1) / a.TI;
  a.work = outer * a.tiles;                                     // <= outer inner, checked above
  a.CP = group_rows_pass(a.TI);
  if (a.CP > chunks) a.CP = chunks > 1 ? chunks : 1;            // fewer chunks than a pass holds
  const size_t lds = (size_t)(a.CP + 2) * a.TI * 8 + (size_t)(G + 1 + RS_THREADS) * 4;
  FTN_CHECK_ARG(lds <= 65536, "%s: a tile of %d columns takes %zu bytes of LDS", who, a.TI, lds);
  const dim3 grid((unsigned)(a.work < RS_GRID_MAX ? a.work : RS_GRID_MAX));
  hipStream_t st = (hipStream_t)stream;
  if (form & FTN_SHELL_VEC) hipLaunchKernelGGL(k_group_sum_rows<true>, grid, dim3(RS_THREADS), lds, st, a);
  else hipLaunchKernelGGL(k_group_sum_rows<false>, grid, dim3(RS_THREADS), lds, st, a);
  FTN_CHECK_LAUNCH();
  return 0;
}
