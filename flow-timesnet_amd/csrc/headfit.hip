// Refitting the heads under the model's own loss (reference losses.py:27-58 under autograd): the gradient of the
// negative-binomial likelihood with respect to rate and dispersion, where the forecast lies.
//   k_nb_grad<V>     one pass over y, rate, dispersion (and a mask): the log-likelihood's derivatives per element,
//                    and per workgroup the partial sums of ll w and of w
//   k_nb_grad_fold   adds the partials in ascending order, writes loss = -sum(ll w) / max(sum w, 1) and the scale
//                    -1 / max(sum w, 1), and (when asked) multiplies the derivatives by that scale in place
// Arithmetic is fp64 (ftn_nbmath.h), reads and writes are fp32.  The dispersion derivative
//   (log1p(alpha mu) - [psi(y + 1/alpha) - psi(1/alpha)]) / alpha^2 + (y - mu) / (alpha (1 + alpha mu))
// cancels to a remainder 1 / (alpha mu) below its terms; in fp32 under autograd nothing of it is left near the
// dispersion floor.  Every sum is taken in an order the shape fixes: a thread over its elements ascending, the
// threads of a workgroup in a fixed tree, the workgroups ascending.  No atomics; every workgroup of the fold
// computes the same two words.
#include "ftn_common.h"
#include "ftn_nbmath.h"

#define NBG_BLOCK 256

struct NbGradArgs {
  const float* y;  const float* rate;  const float* disp;
  const void* mask;            // [B][H][N] contiguous: uint8 (mask_kind 1) or fp32 (2); null (0)
  float* g_rate;  float* g_disp;   // [B][H][N] contiguous
  double* part;                // [gridDim.x][2]
  long long ybs, rbs, dbs;     // batch strides in elements
  long long HN;
  float eps;
  int B, mask_kind;
};

// One element: the derivatives of its log-likelihood (0 where the clamp at eps is active), the log-likelihood itself
// and whether it counts.  The validity rule is sc_element's (score.hip), which is the reference's.
__device__ inline void nbg_element(float y, float rate, float disp, bool m, float eps, float& gr, float& gd,
                                   double& ll, bool& valid) {
  const float yc = y < 0.f ? 0.f : y;                           // comparisons, not fmaxf: a NaN stays a NaN
  const float al = disp < eps ? eps : disp;
  const float mu = rate < eps ? eps : rate;
  valid = m && __builtin_isfinite(yc) && __builtin_isfinite(al) && __builtin_isfinite(mu);
  gr = 0.f;
  gd = 0.f;
  ll = 0.0;
  if (valid) {
    const double A = (double)al, M = (double)mu, r = sc_rcp(A), t = A * M;   // the product of two floats is exact
    double l1p;
    ll = sc_nb_ll((double)yc, r, t, l1p);
    const double dq = ((double)yc - M) * sc_rcp(1.0 + t);       // (y - mu) / (1 + alpha mu)
    if (!(rate < eps)) gr = (float)(dq * sc_rcp(M));
    if (!(disp < eps)) gd = (float)fma((l1p - sc_dpsi((double)yc, r)) * r, r, dq * r);
  }
}

// The sums of a workgroup's 256 threads, in a fixed tree; the result in thread 0.
__device__ inline void nbg_block_sum(double& a, double& b, double* s_a, double* s_b) {
  s_a[threadIdx.x] = a;
  s_b[threadIdx.x] = b;
  __syncthreads();
#pragma unroll
  for (int w = NBG_BLOCK / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      s_a[threadIdx.x] += s_a[threadIdx.x + w];
      s_b[threadIdx.x] += s_b[threadIdx.x + w];
    }
    __syncthreads();
  }
  a = s_a[0];
  b = s_b[0];
}

template <int V>
__global__ __launch_bounds__(NBG_BLOCK) void k_nb_grad(NbGradArgs a) {
  __shared__ double s_ll[NBG_BLOCK], s_w[NBG_BLOCK];
  const long long upb = a.HN / V, units = upb * a.B;            // V == 4: HN % 4 == 0, a quad has one b
  double sll = 0.0, sw = 0.0;
  for (long long u = (long long)blockIdx.x * NBG_BLOCK + threadIdx.x; u < units; u += (long long)gridDim.x * NBG_BLOCK) {
    const long long b = u / upb, i = (u - b * upb) * V;
    const size_t o = (size_t)b * a.HN + i;                      // into mask and the outputs
    const float* __restrict__ yp = a.y + (size_t)b * a.ybs + i;
    const float* __restrict__ rp = a.rate + (size_t)b * a.rbs + i;
    const float* __restrict__ dp = a.disp + (size_t)b * a.dbs + i;
    float y[V], rt[V], ds[V], gr[V], gd[V];
    bool m[V];
    if (V == 4) {
      const f4 yv = *(const f4*)yp, rv = *(const f4*)rp, dv = *(const f4*)dp;
      uint32_t mb = 0x01010101u;
      f4 mf = {1.f, 1.f, 1.f, 1.f};
      if (a.mask_kind == 1) mb = *(const uint32_t*)((const uint8_t*)a.mask + o);
      if (a.mask_kind == 2) mf = *(const f4*)((const float*)a.mask + o);
#pragma unroll
      for (int k = 0; k < V; ++k) {
        y[k] = yv[k]; rt[k] = rv[k]; ds[k] = dv[k];
        m[k] = ((mb >> (8 * k)) & 0xffu) != 0 && mf[k] != 0.f;
      }
    } else {
      y[0] = yp[0]; rt[0] = rp[0]; ds[0] = dp[0];
      m[0] = a.mask_kind == 1 ? ((const uint8_t*)a.mask)[o] != 0
           : a.mask_kind == 2 ? ((const float*)a.mask)[o] != 0.f : true;
    }
#pragma unroll
    for (int k = 0; k < V; ++k) {
      double ll;
      bool valid;
      nbg_element(y[k], rt[k], ds[k], m[k], a.eps, gr[k], gd[k], ll, valid);
      if (valid) { sll += ll; sw += 1.0; }
    }
    if (V == 4) {
      *(f4*)(a.g_rate + o) = f4{gr[0], gr[1], gr[2], gr[3]};
      *(f4*)(a.g_disp + o) = f4{gd[0], gd[1], gd[2], gd[3]};
    } else {
      a.g_rate[o] = gr[0];
      a.g_disp[o] = gd[0];
    }
  }
  nbg_block_sum(sll, sw, s_ll, s_w);
  if (threadIdx.x == 0) {
    a.part[2 * (size_t)blockIdx.x] = sll;
    a.part[2 * (size_t)blockIdx.x + 1] = sw;
  }
}

// out[0] = loss, out[1] = -1 / max(sum w, 1).  Thread t adds partials t, t + 256, ... ascending, then the tree: the
// same words in every workgroup, so each scales its own share of the derivatives with no second synchronisation.
__global__ __launch_bounds__(NBG_BLOCK) void k_nb_grad_fold(const double* __restrict__ part, int nparts, float* out,
                                                            float* g_rate, float* g_disp, long long elems) {
  __shared__ double s_ll[NBG_BLOCK], s_w[NBG_BLOCK];
  double sll = 0.0, sw = 0.0;
  for (int p = threadIdx.x; p < nparts; p += NBG_BLOCK) {
    sll += part[2 * (size_t)p];
    sw += part[2 * (size_t)p + 1];
  }
  nbg_block_sum(sll, sw, s_ll, s_w);
  const double inv = -sc_rcp(sw < 1.0 ? 1.0 : sw);
  const float scale = (float)inv;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    out[0] = (float)(sll * inv);
    out[1] = scale;
  }
  if (g_rate == nullptr) return;
  for (long long e = (long long)blockIdx.x * NBG_BLOCK + threadIdx.x; e < elems; e += (long long)gridDim.x * NBG_BLOCK) {
    g_rate[e] *= scale;
    g_disp[e] *= scale;
  }
}

// The form ftn_nb_nll_grad takes (include/flowtimes.h): the one place the choice is made.
static int nb_grad_form(int B, long long HN, long long ybs, long long rbs, long long dbs, unsigned misalign_or) {
  const bool vec = HN % 4 == 0 && ftn_vec4_ok(4, ybs, rbs, dbs, misalign_or);
  const long long units = B * (vec ? HN / 4 : HN);
  long long nparts = (units + NBG_BLOCK - 1) / NBG_BLOCK;
  if (nparts > FTN_NBG_PARTS_MAX) nparts = FTN_NBG_PARTS_MAX;
  return (vec ? FTN_SHELL_VEC : 0) | (int)nparts << 4;
}

static bool nb_grad_shape_ok(int B, int H, int N) {
  return B >= 1 && H >= 1 && N >= 1 && (long long)H * N <= 0x7fffffffLL && (long long)B * N <= 0x7fffffffLL;
}

extern "C" int ftn_nb_nll_grad_form(int B, int H, int N, long long y_bstride, long long rate_bstride,
                                    long long disp_bstride, int misalign_or) {
  FTN_CHECK_ARG(nb_grad_shape_ok(B, H, N), "ftn_nb_nll_grad_form: B=%d H=%d N=%d", B, H, N);
  FTN_CHECK_ARG(y_bstride >= 0 && rate_bstride >= 0 && disp_bstride >= 0 && misalign_ok(misalign_or),
                "ftn_nb_nll_grad_form: strides %lld %lld %lld misalign=%d", y_bstride, rate_bstride, disp_bstride,
                misalign_or);
  return nb_grad_form(B, (long long)H * N, y_bstride, rate_bstride, disp_bstride, (unsigned)misalign_or);
}

extern "C" size_t ftn_nb_nll_grad_workspace(int B, int H, int N) {
  if (!nb_grad_shape_ok(B, H, N)) return 0;
  return (size_t)(nb_grad_form(B, (long long)H * N, 0, 0, 0, 1) >> 4) * 2 * sizeof(double);   // the scalar form's grid
}

extern "C" int ftn_nb_nll_grad(const float* y_dev, long long y_bstride, const float* rate_dev, long long rate_bstride,
                               const float* disp_dev, long long disp_bstride, const void* mask_dev, int mask_kind,
                               float eps, int B, int H, int N, float* g_rate_dev, float* g_disp_dev, float* loss_dev,
                               void* workspace_dev, size_t workspace_bytes, int scaled, void* stream) {
  FTN_CHECK_ARG(y_dev && rate_dev && disp_dev && g_rate_dev && g_disp_dev && loss_dev && workspace_dev,
                "ftn_nb_nll_grad: null pointer");
  FTN_CHECK_ARG(nb_grad_shape_ok(B, H, N), "ftn_nb_nll_grad: bad shape B=%d H=%d N=%d", B, H, N);
  const long long row = (long long)H * N;
  FTN_CHECK_ARG(y_bstride >= 0 && rate_bstride >= 0 && disp_bstride >= 0, "ftn_nb_nll_grad: negative batch stride");
  FTN_CHECK_ARG(B == 1 || (y_bstride >= row && rate_bstride >= row && disp_bstride >= row),
                "ftn_nb_nll_grad: batch strides %lld %lld %lld are below H N = %lld", y_bstride, rate_bstride,
                disp_bstride, row);
  FTN_CHECK_ARG(mask_kind >= 0 && mask_kind <= 2 && (mask_kind == 0) == (mask_dev == nullptr),
                "ftn_nb_nll_grad: mask_kind=%d does not fit the mask pointer", mask_kind);
  FTN_CHECK_ARG(eps > 0.f && eps < 1.f, "ftn_nb_nll_grad: eps=%g", (double)eps);
  FTN_CHECK_ARG(scaled == 0 || scaled == 1, "ftn_nb_nll_grad: scaled=%d", scaled);
  const uintptr_t ptrs = (uintptr_t)y_dev | (uintptr_t)rate_dev | (uintptr_t)disp_dev | (uintptr_t)g_rate_dev |
                         (uintptr_t)g_disp_dev;
  FTN_CHECK_ARG((ptrs & 3) == 0 && ((uintptr_t)loss_dev & 3) == 0 && (mask_kind != 2 || ((uintptr_t)mask_dev & 3) == 0) &&
                    ((uintptr_t)workspace_dev & 7) == 0,
                "ftn_nb_nll_grad: operands must be 4-byte aligned, the workspace 8-byte aligned");
  FTN_CHECK_ARG(g_rate_dev != g_disp_dev, "ftn_nb_nll_grad: g_rate and g_disp are one buffer");
  unsigned mis = (unsigned)(ptrs & 15);
  if (mask_kind == 2) mis |= (unsigned)((uintptr_t)mask_dev & 15);
  if (mask_kind == 1) mis |= (unsigned)((uintptr_t)mask_dev & 3) << 2;
  const int form = nb_grad_form(B, row, B > 1 ? y_bstride : 0, B > 1 ? rate_bstride : 0, B > 1 ? disp_bstride : 0, mis);
  const int nparts = form >> 4;
  FTN_CHECK_ARG(workspace_bytes >= (size_t)nparts * 2 * sizeof(double),
                "ftn_nb_nll_grad: workspace of %zu bytes, %zu needed (ftn_nb_nll_grad_workspace)", workspace_bytes,
                (size_t)nparts * 2 * sizeof(double));
  NbGradArgs a;
  a.y = y_dev; a.rate = rate_dev; a.disp = disp_dev; a.mask = mask_dev; a.g_rate = g_rate_dev; a.g_disp = g_disp_dev;
  a.part = (double*)workspace_dev;
  a.ybs = B > 1 ? y_bstride : 0; a.rbs = B > 1 ? rate_bstride : 0; a.dbs = B > 1 ? disp_bstride : 0;
  a.HN = row; a.eps = eps; a.B = B; a.mask_kind = mask_kind;
  hipStream_t st = (hipStream_t)stream;
  if (form & FTN_SHELL_VEC) hipLaunchKernelGGL(k_nb_grad<4>, dim3((unsigned)nparts), dim3(NBG_BLOCK), 0, st, a);
  else hipLaunchKernelGGL(k_nb_grad<1>, dim3((unsigned)nparts), dim3(NBG_BLOCK), 0, st, a);
  FTN_CHECK_LAUNCH();
  const long long elems = (long long)B * row;
  long long fold = scaled ? (elems + NBG_BLOCK - 1) / NBG_BLOCK : 1;
  if (fold > FTN_NBG_PARTS_MAX) fold = FTN_NBG_PARTS_MAX;
  hipLaunchKernelGGL(k_nb_grad_fold, dim3((unsigned)fold), dim3(NBG_BLOCK), 0, st, (const double*)a.part, nparts, loss_dev,
                     scaled ? g_rate_dev : nullptr, scaled ? g_disp_dev : nullptr, elems);
  FTN_CHECK_LAUNCH();
  return 0;
}

// ---------------------------------------------------------------------------------------------
// The heads for a refit: a forward that keeps the two sigmoids, and the backward
// ---------------------------------------------------------------------------------------------
//   (forward)           the head kernels themselves (shell.hip, shell_wide.hip: same forms, same rate and dispersion
//                       bits), which store softplus' derivative at both pre-activations when HeadArgs asks:
//                       sigmoid(t) for t <= 20, 1 above
//   k_headfit_colsum    N <= 4: lanes own float4 columns of hidden, a workgroup sums the rows of its chunk
//   k_headfit_mfma      otherwise: a wave owns a [32 n x 32 d] tile of both heads, K = the rows of its chunk, on
//                       v_mfma_f32_32x32x2_f32 (a bitwise fmaf chain: no operand is split).  G is read with n along
//                       the lanes and hidden with d along the lanes: both coalesced, no transpose.
//   k_headfit_reduce    adds the chunks' partials in ascending order into dW and db
//   k_headfit_dhidden   d_hidden = G_mu W_mu + G_sg W_sg, when asked
// G = g * sigma' * scale with g the raw derivatives and scale the device word of ftn_nb_nll_grad, formed where it is
// used.  A chunk's partial is [2 heads][N][D + 1], column D the bias (the MFMA form multiplies G by a column of
// ones).  Every sum's order is a function of (R, N, D) alone and every word of the workspace that is read was
// written by this call.
#include "ftn_shell.h"

#define HF_CHUNK 256

struct HeadBwdArgs {
  const float* hidden;                     // [R][D]
  const float* g_rate;  const float* g_disp;   // raw derivatives [R][N]
  const float* sig_mu;  const float* sig_sg;   // softplus' derivative [R][N]
  const float* scale;                      // one device word
  const float* wmu;  const float* wsg;     // [N][D], for d_hidden
  float* part;                             // [chunks][2][N][D + 1]
  float* dwmu;  float* dbmu;  float* dwsg;  float* dbsg;
  float* dhidden;                          // [R][D] or null
  long long R;
  int N, D, chunk, chunks;
};

// N <= 4.  Thread t: float4 column q = t % DQ of hidden, row lane j = t / DQ of JN = 256 / DQ; rows j, j + JN, ...
// of the chunk ascending, then the row lanes added in ascending order by j = 0.  Column D (the bias) by q = 0.
template <int NN>
__global__ __launch_bounds__(256) void k_headfit_colsum(HeadBwdArgs a) {
  extern __shared__ float s_acc[];                              // [JN][2 NN][D + 1]
  const int DQ = a.D >> 2, JN = 256 / DQ, q = threadIdx.x % DQ, j = threadIdx.x / DQ, W = a.D + 1;
  const long long r0 = (long long)blockIdx.x * a.chunk, r1 = r0 + a.chunk < a.R ? r0 + a.chunk : a.R;
  const float scale = *a.scale;
  f4 acc[2 * NN];
  float bias[2 * NN];
#pragma unroll
  for (int k = 0; k < 2 * NN; ++k) { acc[k] = f4{0.f, 0.f, 0.f, 0.f}; bias[k] = 0.f; }
  if (j < JN) {
    for (long long r = r0 + j; r < r1; r += JN) {
      const f4 h = *(const f4*)(a.hidden + r * a.D + 4 * q);
#pragma unroll
      for (int n = 0; n < NN; ++n) {
        const size_t at = (size_t)r * NN + n;
        const float gm = a.g_rate[at] * a.sig_mu[at] * scale, gs = a.g_disp[at] * a.sig_sg[at] * scale;
        acc[n] += gm * h;
        acc[NN + n] += gs * h;
        bias[n] += gm;
        bias[NN + n] += gs;
      }
    }
#pragma unroll
    for (int k = 0; k < 2 * NN; ++k) {
      float* row = s_acc + ((size_t)j * 2 * NN + k) * W;
#pragma unroll
      for (int e = 0; e < 4; ++e) row[4 * q + e] = acc[k][e];
      if (q == 0) row[a.D] = bias[k];
    }
  }
  __syncthreads();
  float* out = a.part + (size_t)blockIdx.x * 2 * NN * W;
  for (int i = threadIdx.x; i < 2 * NN * W; i += 256) {
    float v = 0.f;
    for (int jj = 0; jj < JN; ++jj) v += s_acc[(size_t)jj * 2 * NN * W + i];
    out[i] = v;
  }
}

// One wave: tile (tn, td) of chunk blockIdx.y.  A[i = n][k = row] = G, B[k = row][j = d] = hidden (1 at d == D).
__global__ __launch_bounds__(64) void k_headfit_mfma(HeadBwdArgs a) {
  const int W = a.D + 1, dtiles = (W + 31) >> 5;
  const int tn = blockIdx.x / dtiles, td = blockIdx.x - tn * dtiles;
  const int lane = threadIdx.x, k = lane >> 5, n = tn * 32 + (lane & 31), d = td * 32 + (lane & 31);
  const long long r0 = (long long)blockIdx.y * a.chunk, r1 = r0 + a.chunk < a.R ? r0 + a.chunk : a.R;
  const float scale = *a.scale;
  const bool nok = n < a.N, dok = d < a.D;
  f16v cm, cs;
#pragma unroll
  for (int e = 0; e < 16; ++e) { cm[e] = 0.f; cs[e] = 0.f; }
  for (long long r = r0 + k; r < r1 + k; r += 2) {              // both halves of the wave take every step
    const bool rok = r < r1;
    float gm = 0.f, gs = 0.f, h = 0.f;
    if (rok && nok) {
      const size_t at = (size_t)r * a.N + n;
      gm = a.g_rate[at] * a.sig_mu[at] * scale;
      gs = a.g_disp[at] * a.sig_sg[at] * scale;
    }
    if (rok) h = dok ? a.hidden[r * a.D + d] : (d == a.D ? 1.f : 0.f);
    cm = __builtin_amdgcn_mfma_f32_32x32x2f32(gm, h, cm, 0, 0, 0);
    cs = __builtin_amdgcn_mfma_f32_32x32x2f32(gs, h, cs, 0, 0, 0);
  }
  // C/D: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
  float* out = a.part + (size_t)blockIdx.y * 2 * a.N * W;
  if (d < W) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int nn = tn * 32 + (e & 3) + 8 * (e >> 2) + 4 * k;
      if (nn < a.N) {
        out[(size_t)nn * W + d] = cm[e];
        out[((size_t)a.N + nn) * W + d] = cs[e];
      }
    }
  }
}

__global__ __launch_bounds__(256) void k_headfit_reduce(HeadBwdArgs a) {
  const int W = a.D + 1;
  const long long per = (long long)2 * a.N * W, i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= per) return;
  float v = 0.f;
  for (int c = 0; c < a.chunks; ++c) v += a.part[(size_t)c * per + i];
  const int head = (int)(i / ((long long)a.N * W));
  const long long rest = i - (long long)head * a.N * W;
  const int n = (int)(rest / W), d = (int)(rest - (long long)n * W);
  if (d == a.D) (head ? a.dbsg : a.dbmu)[n] = v;
  else (head ? a.dwsg : a.dwmu)[(size_t)n * a.D + d] = v;
}

__global__ __launch_bounds__(256) void k_headfit_dhidden(HeadBwdArgs a) {
  const int DQ = a.D >> 2;
  const long long total = a.R * DQ;
  const float scale = *a.scale;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long r = i / DQ;
    const int d = (int)(i - r * DQ) * 4;
    f4 v = {0.f, 0.f, 0.f, 0.f};
    for (int n = 0; n < a.N; ++n) {
      const size_t at = (size_t)r * a.N + n;
      const float gm = a.g_rate[at] * a.sig_mu[at] * scale, gs = a.g_disp[at] * a.sig_sg[at] * scale;
      v += gm * *(const f4*)(a.wmu + (size_t)n * a.D + d);
      v += gs * *(const f4*)(a.wsg + (size_t)n * a.D + d);
    }
    *(f4*)(a.dhidden + r * a.D + d) = v;
  }
}

// The form ftn_head_backward takes: the one place the choice is made.  Chunks of HF_CHUNK rows, at most
// FTN_HEADFIT_CHUNKS_MAX of them: beyond that the chunk grows (to an even number of rows).
static int head_bwd_chunk(long long R) {
  long long c = HF_CHUNK;
  if ((R + c - 1) / c > FTN_HEADFIT_CHUNKS_MAX) {
    c = (R + FTN_HEADFIT_CHUNKS_MAX - 1) / FTN_HEADFIT_CHUNKS_MAX;
    c += c & 1;
  }
  return (int)c;
}
static bool head_bwd_shape_ok(long long R, int N, int D) {
  return R >= 1 && R <= 0x7fffffffLL && N >= 1 && D >= 4 && D <= 512 && D % 4 == 0 && (long long)R * N <= 0x7fffffffLL * 4 &&
         (long long)N * (D + 1) <= 0x3fffffffLL;
}
static int head_bwd_form(long long R, int N, int D, unsigned misalign_or) {
  const int chunk = head_bwd_chunk(R), chunks = (int)((R + chunk - 1) / chunk);
  const bool colsum = N <= 4 && (misalign_or & 15) == 0;
  return (colsum ? FTN_HEADFIT_COLSUM : FTN_HEADFIT_MFMA) | chunks << 4;
}

extern "C" int ftn_head_backward_form(long long R, int N, int D, int misalign_or) {
  FTN_CHECK_ARG(head_bwd_shape_ok(R, N, D) && misalign_ok(misalign_or),
                "ftn_head_backward_form: R=%lld N=%d d_model=%d misalign=%d", R, N, D, misalign_or);
  return head_bwd_form(R, N, D, (unsigned)misalign_or);
}

extern "C" size_t ftn_head_backward_workspace(long long R, int N, int D) {
  if (!head_bwd_shape_ok(R, N, D)) return 0;
  return (size_t)(head_bwd_form(R, N, D, 0) >> 4) * 2 * N * (D + 1) * sizeof(float);
}

extern "C" int ftn_head_fit_forward(const float* hidden_dev, long long rows, int S, int D, int N, const float* w_mu_dev,
                                    const float* b_mu_dev, const float* w_sigma_dev, const float* b_sigma_dev,
                                    const float* tail_dev, long long tail_bstride, int hist,
                                    const float* late_dev_or_null, long long late_bstride,
                                    const float* floor_vec_dev_or_null, float floor_scalar, float* rate_dev,
                                    float* disp_dev, float* sig_mu_dev, float* sig_sigma_dev, int* bad_flag_dev,
                                    void* stream) {
  const char* who = "ftn_head_fit_forward";
  FTN_CHECK_ARG(hidden_dev && w_mu_dev && b_mu_dev && w_sigma_dev && b_sigma_dev && tail_dev && rate_dev && disp_dev &&
                    sig_mu_dev && sig_sigma_dev && bad_flag_dev, "%s: null pointer", who);
  FTN_CHECK_ARG(rows >= 1 && S >= 1 && rows % S == 0 && N >= 1 && hist >= 1 && hist <= S && head_bwd_shape_ok(rows, N, D),
                "%s: rows=%lld S=%d N=%d hist=%d d_model=%d", who, rows, S, N, hist, D);
  FTN_CHECK_ARG(tail_bstride >= 0 && late_bstride >= 0, "%s: negative batch stride", who);
  FTN_CHECK_ARG((((uintptr_t)hidden_dev | (uintptr_t)w_mu_dev | (uintptr_t)w_sigma_dev) & 15) == 0,
                "%s: hidden and the head weights must be 16-byte aligned", who);
  FTN_CHECK_ARG((((uintptr_t)b_mu_dev | (uintptr_t)b_sigma_dev | (uintptr_t)tail_dev | (uintptr_t)late_dev_or_null |
                  (uintptr_t)floor_vec_dev_or_null | (uintptr_t)rate_dev | (uintptr_t)disp_dev |
                  (uintptr_t)bad_flag_dev) & 3) == 0 && (((uintptr_t)sig_mu_dev | (uintptr_t)sig_sigma_dev) & 15) == 0,
                "%s: every operand must be 4-byte aligned, sig_mu and sig_sigma 16-byte", who);
  HeadArgs a;
  a.hidden = hidden_dev; a.wmu = w_mu_dev; a.bmu = b_mu_dev; a.wsg = w_sigma_dev; a.bsg = b_sigma_dev;
  a.tail = tail_dev; a.late = late_dev_or_null; a.floorv = floor_vec_dev_or_null; a.rate = rate_dev; a.disp = disp_dev;
  a.bad = bad_flag_dev; a.rows = rows; a.tail_bs = tail_bstride; a.late_bs = late_bstride;
  a.S = S; a.D = D; a.N = N; a.hist = hist; a.floor_s = floor_scalar;
  a.sig_mu = sig_mu_dev; a.sig_sg = sig_sigma_dev;
  return (D > 128 ? head_wide_launch : head_launch)(a, (hipStream_t)stream);
}

extern "C" int ftn_head_backward(const float* hidden_dev, long long R, int N, int D, const float* g_rate_dev,
                                 const float* g_disp_dev, const float* sig_mu_dev, const float* sig_sigma_dev,
                                 const float* scale_dev, const float* w_mu_dev, const float* w_sigma_dev,
                                 float* dw_mu_dev, float* db_mu_dev, float* dw_sigma_dev, float* db_sigma_dev,
                                 float* d_hidden_dev_or_null, void* workspace_dev, size_t workspace_bytes,
                                 void* stream) {
  const char* who = "ftn_head_backward";
  FTN_CHECK_ARG(hidden_dev && g_rate_dev && g_disp_dev && sig_mu_dev && sig_sigma_dev && scale_dev && dw_mu_dev &&
                    db_mu_dev && dw_sigma_dev && db_sigma_dev && workspace_dev, "%s: null pointer", who);
  FTN_CHECK_ARG(!d_hidden_dev_or_null || (w_mu_dev && w_sigma_dev), "%s: d_hidden needs both weights", who);
  FTN_CHECK_ARG(head_bwd_shape_ok(R, N, D), "%s: R=%lld N=%d d_model=%d (a multiple of 4, <= 512)", who, R, N, D);
  FTN_CHECK_ARG((((uintptr_t)hidden_dev | (uintptr_t)g_rate_dev | (uintptr_t)g_disp_dev | (uintptr_t)sig_mu_dev |
                  (uintptr_t)sig_sigma_dev | (uintptr_t)scale_dev | (uintptr_t)dw_mu_dev | (uintptr_t)db_mu_dev |
                  (uintptr_t)dw_sigma_dev | (uintptr_t)db_sigma_dev | (uintptr_t)workspace_dev) & 3) == 0,
                "%s: every operand must be 4-byte aligned", who);
  FTN_CHECK_ARG(!d_hidden_dev_or_null ||
                    (((uintptr_t)d_hidden_dev_or_null | (uintptr_t)w_mu_dev | (uintptr_t)w_sigma_dev) & 15) == 0,
                "%s: d_hidden and the head weights must be 16-byte aligned", who);
  const int form = head_bwd_form(R, N, D, (unsigned)((uintptr_t)hidden_dev & 15));
  HeadBwdArgs a;
  a.hidden = hidden_dev; a.g_rate = g_rate_dev; a.g_disp = g_disp_dev; a.sig_mu = sig_mu_dev; a.sig_sg = sig_sigma_dev;
  a.scale = scale_dev; a.wmu = w_mu_dev; a.wsg = w_sigma_dev; a.part = (float*)workspace_dev;
  a.dwmu = dw_mu_dev; a.dbmu = db_mu_dev; a.dwsg = dw_sigma_dev; a.dbsg = db_sigma_dev; a.dhidden = d_hidden_dev_or_null;
  a.R = R; a.N = N; a.D = D; a.chunk = head_bwd_chunk(R); a.chunks = form >> 4;
  const size_t need = (size_t)a.chunks * 2 * N * (D + 1) * sizeof(float);
  FTN_CHECK_ARG(workspace_bytes >= need, "%s: workspace of %zu bytes, %zu needed (ftn_head_backward_workspace)", who,
                workspace_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  if ((form & 15) == FTN_HEADFIT_COLSUM) {
    const size_t lds = (size_t)(256 / (D / 4)) * 2 * N * (D + 1) * sizeof(float);
    void (*kern)(HeadBwdArgs) = N == 1 ? k_headfit_colsum<1> : N == 2 ? k_headfit_colsum<2> : N == 3 ? k_headfit_colsum<3>
                                                                                                  : k_headfit_colsum<4>;
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) { ftn_set_error("hipFuncSetAttribute(k_headfit_colsum): %s", hipGetErrorString(e)); return (int)e; }
    hipLaunchKernelGGL(kern, dim3((unsigned)a.chunks), dim3(256), lds, st, a);
  } else {
    const int tiles = ((N + 31) / 32) * ((D + 1 + 31) / 32);
    hipLaunchKernelGGL(k_headfit_mfma, dim3((unsigned)tiles, (unsigned)a.chunks), dim3(64), 0, st, a);
  }
  FTN_CHECK_LAUNCH();
  const long long per = (long long)2 * N * (D + 1);
  hipLaunchKernelGGL(k_headfit_reduce, dim3((unsigned)((per + 255) / 256)), dim3(256), 0, st, a);
  FTN_CHECK_LAUNCH();
  if (d_hidden_dev_or_null) {
    long long nblk = (R * (D / 4) + 255) / 256;
    if (nblk > 4096) nblk = 4096;
    hipLaunchKernelGGL(k_headfit_dhidden, dim3((unsigned)nblk), dim3(256), 0, st, a);
    FTN_CHECK_LAUNCH();
  }
  return 0;
}
