// Series groups: out[row][g] = the sum of x[row][i] over the members i of group g, the groups given as CSR member
// lists (include/flowtimes.h states the definition to the bit: chunks of 32 members in fp64 left to right, the chunk
// sums in ascending order in fp64, one rounding).  One read of x from HBM, nothing intermediate there.
//
// k_group_sum<VEC>: a workgroup walks tiles of T rows (tile = blockIdx.x, + gridDim.x, ..).  Once, it forms the first
// chunk of every group (cfirst [G + 1], a prefix sum over the device offsets) in LDS.  Per tile it
//   stages   the T rows into LDS with coalesced 16-byte (VEC) or 4-byte loads, element i at word i + (i >> 5) of its
//            row: ds_read_b32 banks are (word % 32) per 32-lane half, and for groups of consecutive series lane c
//            reads element 32 c + j - one bank unpadded, 32 banks at 33 c + j;
//   sums     work items (row, chunk), chunk fastest along the lanes: an item holds the LDS words of its chunk's <= 32
//            members in registers (read from `order` once per workgroup when the chunks fit the lanes, else once per
//            tile) and adds them in fp64 for the rows r, r + RG, ..; a member slot beyond the chunk's end points at a
//            zero word that ends every staged row - a sum that starts at +0.0 is never -0.0, so adding +0.0 changes
//            no bit and the walk has no branch;
//   combines one thread per (row, group), group fastest: that group's chunk sums in ascending order, rounded, stored.
// Neither the tile height, the grid nor the load width enters a group's sum.  The device CSR is read through
// ftn_groups.h alone, which clamps what it reads, and a member outside 0 .. N - 1 points at the zero word, so a CSR
// that disagrees with the validated host copy cannot address anything outside x, order, out and the workgroup's LDS.
#include "ftn_groups.h"

#define GS_THREADS 256
#define GS_GRID_MAX 1024

struct GroupArgs {
  const float* x;  float* out;  FtnGroupCsr csr;
  long long rows, stride, tiles;
  int N, T, pitch, clsh;            // T rows a tile, pitch words a staged row, 2^clsh lanes along chunks
};

static inline int gs_pitch(int N) { return N + (N >> 5) + 1; }

// The form every entry point takes (include/flowtimes.h): the one place the choice is made.
static inline int group_form(int N, long long stride, unsigned misalign, int C) {
  const bool vec = N % 4 == 0 && stride % 4 == 0 && (misalign & 15) == 0;
  const long long row_bytes = 4LL * gs_pitch(N) + 8LL * C;
  long long T = FTN_GROUP_TILE_BYTES / row_bytes;
  T = T > FTN_GROUP_TILE_ROWS ? FTN_GROUP_TILE_ROWS : T < 1 ? 1 : T;
  return (vec ? FTN_SHELL_VEC : 0) | (int)T << 8;
}

// the LDS words (relative to a staged row) of chunk c's members; slots beyond its end are the row's zero word
__device__ __forceinline__ void gs_members(const GroupArgs& a, const int* cfirst, int c, int (&pos)[FTN_GROUP_CHUNK]) {
  const FtnGroupChunk k = ftn_csr_chunk(a.csr, cfirst, c);
#pragma unroll
  for (int j = 0; j < FTN_GROUP_CHUNK; ++j) {
    const int i = j < k.len ? a.csr.order[k.start + j] : -1;
    pos[j] = (unsigned)i < (unsigned)a.N ? i + (i >> 5) : a.pitch - 1;
  }
}

__device__ __forceinline__ void gs_sums(const GroupArgs& a, const float* rowsm, double* csum, int c, int rg, int RG,
                                        int live, const int (&pos)[FTN_GROUP_CHUNK]) {
  for (int r = rg; r < live; r += RG) {
    const float* row = rowsm + r * a.pitch;
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < FTN_GROUP_CHUNK; ++j) acc += (double)row[pos[j]];
    csum[r * a.csr.C + c] = acc;
  }
}

// element i of a row sits at word i + (i >> 5); a quad (v = i / 4) lies inside one block of 32
template <bool VEC>
__device__ __forceinline__ void gs_stage(float* row, int v, f4 q) {
  float* d = row + 4 * v + (v >> 3);
  d[0] = q.x; d[1] = q.y; d[2] = q.z; d[3] = q.w;
}
template <bool VEC>
__device__ __forceinline__ void gs_stage(float* row, int v, float q) { row[v + (v >> 5)] = q; }

template <bool VEC>
__global__ __launch_bounds__(GS_THREADS) void k_group_sum(GroupArgs a) {
  using Ld = typename std::conditional<VEC, f4, float>::type;
  constexpr int W = VEC ? 4 : 1;
  extern __shared__ __attribute__((aligned(16))) unsigned char gs_lds[];
  double* csum = (double*)gs_lds;                               // [T][C]
  int* cfirst = (int*)(csum + (size_t)a.T * a.csr.C);           // [G + 1]
  int* part = cfirst + a.csr.G + 1;                             // [GS_THREADS]
  float* rowsm = (float*)(part + GS_THREADS);                   // [T][pitch]
  const int tid = threadIdx.x;

  for (int r = tid; r < a.T; r += GS_THREADS) rowsm[r * a.pitch + a.pitch - 1] = 0.f;
  ftn_csr_first_wg(a.csr, GS_THREADS, part, cfirst);

  const int CL = 1 << a.clsh, cl = tid & (CL - 1), rg = tid >> a.clsh, RG = GS_THREADS >> a.clsh;
  const bool once = a.csr.C <= CL;                          // every chunk has its lane: the members stay in registers
  int pos[FTN_GROUP_CHUNK];
  if (once && cl < a.csr.C) gs_members(a, cfirst, cl, pos);

  // staging: 2^lsh lanes along a row, the rows r0, r0 + RS, ..
  const int nv = VEC ? a.N >> 2 : a.N;
  int lsh = 0;
  while ((1 << lsh) < nv && lsh < 8) ++lsh;
  const int v0 = tid & ((1 << lsh) - 1), r0 = tid >> lsh, RS = GS_THREADS >> lsh;

  for (long long tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
    const long long row0 = tile * a.T;
    const int live = a.rows - row0 < a.T ? (int)(a.rows - row0) : a.T;
    for (int r = r0; r < live; r += RS) {
      const float* src = a.x + (row0 + r) * a.stride;
      float* dst = rowsm + r * a.pitch;
      for (int v = v0; v < nv; v += 1 << lsh) gs_stage<VEC>(dst, v, *(const Ld*)(src + v * W));
    }
    __syncthreads();
    if (once) {
      if (cl < a.csr.C) gs_sums(a, rowsm, csum, cl, rg, RG, live, pos);
    } else {
      for (int c = cl; c < a.csr.C; c += CL) {
        gs_members(a, cfirst, c, pos);
        gs_sums(a, rowsm, csum, c, rg, RG, live, pos);
      }
    }
    __syncthreads();
    for (int w = tid; w < live * a.csr.G; w += GS_THREADS) {
      const int r = w / a.csr.G, g = w - r * a.csr.G;
      const double* s = csum + r * a.csr.C;
      double acc = 0.0;
      for (int k = cfirst[g]; k < cfirst[g + 1]; ++k) acc += s[k];
      a.out[(row0 + r) * a.csr.G + g] = (float)acc;
    }
  }
}

static int group_form_check(const char* who, int N, long long row_stride, int n_chunks) {
  FTN_CHECK_ARG(N >= 1 && N <= FTN_GROUP_NMAX, "%s: N=%d is outside 1..%d", who, N, FTN_GROUP_NMAX);
  FTN_CHECK_ARG(row_stride >= N, "%s: row stride %lld is below N=%d", who, row_stride, N);
  FTN_CHECK_ARG(n_chunks >= 0 && n_chunks <= FTN_GROUP_CHUNKS_MAX, "%s: %d chunks are outside 0..%d", who, n_chunks,
                FTN_GROUP_CHUNKS_MAX);
  return 0;
}

extern "C" int ftn_group_sum_form(int N, long long row_stride, int misalign_or, int n_chunks) {
  if (group_form_check("ftn_group_sum_form", N, row_stride, n_chunks) < 0) return -1;
  FTN_CHECK_ARG(misalign_ok(misalign_or), "ftn_group_sum_form: misalign=%d", misalign_or);
  return group_form(N, row_stride, (unsigned)misalign_or, n_chunks);
}

extern "C" int ftn_group_sum(const float* x_dev, long long rows, int N, long long row_stride, const int* order_dev,
                             const int* offsets_dev, const int* offsets_host, int G, int M, float* out_dev,
                             void* stream) {
  const char* who = "ftn_group_sum";
  int chunks = 0;
  if (group_csr_check(who, x_dev, out_dev, order_dev, offsets_dev, offsets_host, G, M, &chunks) < 0) return -1;
  if (group_form_check(who, N, row_stride, chunks) < 0) return -1;
  FTN_CHECK_ARG(rows >= 1 && rows <= (1LL << 62) / (row_stride > G ? row_stride : G),
                "%s: rows=%lld with stride %lld and G=%d", who, rows, row_stride, G);
  const int form = group_form(N, row_stride, (unsigned)((uintptr_t)x_dev & 15), chunks);
  GroupArgs a = {};
  a.x = x_dev; a.out = out_dev; a.csr = {order_dev, offsets_dev, G, M, chunks};
  a.rows = rows; a.stride = row_stride;
  a.N = N; a.T = form >> 8; a.pitch = gs_pitch(N);
  a.tiles = (rows + a.T - 1) / a.T;
  while ((1 << a.clsh) < a.csr.C && a.clsh < 8) ++a.clsh;
  const size_t lds = (size_t)a.T * ((size_t)a.csr.C * 8 + (size_t)a.pitch * 4) + (size_t)(G + 1 + GS_THREADS) * 4;
  FTN_CHECK_ARG(lds <= 65536, "%s: a tile of %d rows takes %zu bytes of LDS", who, a.T, lds);
  const dim3 grid((unsigned)(a.tiles < GS_GRID_MAX ? a.tiles : GS_GRID_MAX));
  hipStream_t st = (hipStream_t)stream;
  if (form & FTN_SHELL_VEC) hipLaunchKernelGGL(k_group_sum<true>, grid, dim3(GS_THREADS), lds, st, a);
  else hipLaunchKernelGGL(k_group_sum<false>, grid, dim3(GS_THREADS), lds, st, a);
  FTN_CHECK_LAUNCH();
  return 0;
}
