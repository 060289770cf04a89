// TimesBlock conv path on gfx950 (reference models/timesnet.py:955-1101 with the
// inception stack of :560-654, 744-762), v1: one launch per stage, all groups of
// a block call in each launch, intermediates in a caller-provided workspace.
//
// Pixel space.  For group g (period p, pad, cycles) every batch row owns
// P_g = L + pad_g grid pixels t = cycle*p + phase; the period fold of the
// reference (:1041-1046) is exactly this re-indexing of the zero-extended
// window, so no fold pass exists here.  Pixels of all groups are laid out flat,
// group-major: n = B*px_off[g] + b*P_g + t, N = B*total_px.  Activation buffers
// are [N][channels] with channels padded to a multiple of 16.
//
// All contractions run on v_mfma_f32_16x16x4_f32 (exact fp32 FMA chains): rows =
// output channels (A = weights, row-major [out][in]), columns = 16 pixels
// (B = activations).  With the k-order "element e of lane group q is input
// channel 16s+4q+e", the A fragment is one contiguous float4 of the weight row,
// the B fragment one contiguous float4 of the pixel row, and — because result
// register r of lane (j,q) is output channel 4q+r of pixel j — an accumulator
// tile is directly the B fragment of the next 1x1 layer (no LDS, no shuffles).
//
// Stages (bottleneck mode; SURVEY finding 5 folds proj∘branch[-1] into w_out):
//   A  k_pw        a  = W_in1 x + b                  (C -> nbr*mid)
//   B  k_conv      m  = conv_k(a_k) + b              (per branch mid -> mid, zero pad)
//   C  k_mlp       g  = act(act(W_out1 m + b) + res1(x));  a' = W_in2 g + b;  r = res2(g) - x
//   D  k_conv      m' = conv_k(a'_k) + b
//   E+F k_out      y  = x + sum_g w[b,g] * (act(W_out2 m'_g + b) + r_g)[:L]
// Single-conv mode (ratio 1) replaces A by a zero-padded copy of x, B/D by one
// merged conv with proj folded in, and E by an elementwise epilogue.
//
// This unit is the block driver: workspace layout, the form table (block_forms) and the forward that fills the
// stages' argument blocks and calls one launch entry per stage.  The kernels live in stage_a.hip (A, generic C),
// conv.hip (B, D), stagec_px.hip / stagec_pos.hip (C) and stage_out.hip (E + F).
#include <stdlib.h>
#include "ftn_common.h"
#include "ftn_pw.h"
#include "ftn_conv.h"
#include "ftn_mlp.h"
#include "ftn_out.h"
#include "ftn_finalize.h"
#include "ftn_exchange.h"

static const bool g_r_keeps_x = [] { const char* e = getenv("FTN_R_KEEPS_X"); return e == nullptr || e[0] != '0'; }();   // stage C leaves x inside R (default on)
static const bool g_mlp_u1 = [] { const char* e = getenv("FTN_MLP_U1"); return e == nullptr || e[0] != '0'; }();    // 0: the two-unit k_mlp_bf

// ---------------------------------------------------------------- stage timing
// Optional hipEvent brackets around the stages of ftn_timesblock_forward, kept in
// a pool so that nothing synchronises while a timed region runs; read back (with
// one synchronise) by ftn_stage_times.  Used by bench.py for the roofline figures.
#define FTN_NSTAGE 6
#define FTN_PROF_CALLS 512
static struct StageProf {
  bool on = false;
  bool created = false;
  int calls = 0;        // forwards recorded
  int every = 1;        // record every `every`-th forward
  int seen = 0;         // forwards seen since ftn_stage_timing(enable)
  hipEvent_t ev[FTN_PROF_CALLS][FTN_NSTAGE + 1];
  bool sampling() const { return on && calls < FTN_PROF_CALLS && seen % every == 0; }
} g_prof;

static void prof_mark(int stage, hipStream_t st) {
  if (g_prof.sampling()) (void)hipEventRecord(g_prof.ev[g_prof.calls][stage], st);
}

// Diagnostic cycle stamps (ftn_debug_stamps): when a buffer is registered, thread 0 of every workgroup of the selected
// kernels stores s_memtime at its phase boundaries there.  The buffer is read by nothing else; production runs leave
// the pointer null.  which: 1 conv kernels (| 4: stage B only), 2 stage C, 8 the selector's finalize workgroup.
static unsigned long long* g_stamp_buf = nullptr;
static size_t g_stamp_cap = 0;
static int g_stamp_which = 0;

extern "C" int ftn_debug_stamps(void* buf_dev, size_t n_u64, int which) {
  g_stamp_buf = (unsigned long long*)buf_dev;
  g_stamp_cap = buf_dev ? n_u64 : 0;
  g_stamp_which = which;
  return 0;
}

unsigned long long* ftn_stamp_buf(int which_bit, size_t* cap) {
  *cap = g_stamp_cap;
  return (g_stamp_which & which_bit) ? g_stamp_buf : nullptr;
}

extern "C" int ftn_stage_timing(int enable) {
  if (enable && !g_prof.created) {
    for (int c = 0; c < FTN_PROF_CALLS; ++c)
      for (int s = 0; s <= FTN_NSTAGE; ++s) {
        hipError_t e = hipEventCreate(&g_prof.ev[c][s]);
        if (e != hipSuccess) { ftn_set_error("hipEventCreate: %s", hipGetErrorString(e)); return (int)e; }
      }
    g_prof.created = true;
  }
  g_prof.on = enable != 0;
  g_prof.every = enable > 1 ? enable : 1;
  g_prof.calls = 0;
  g_prof.seen = 0;
  return 0;
}

extern "C" int ftn_stage_times(float* ms_sum, int nstage, int* ncalls) {
  FTN_CHECK_ARG(ms_sum && ncalls && nstage == FTN_NSTAGE, "ftn_stage_times: expects %d stages", FTN_NSTAGE);
  for (int s = 0; s < FTN_NSTAGE; ++s) ms_sum[s] = 0.f;
  *ncalls = g_prof.calls;
  for (int c = 0; c < g_prof.calls; ++c) {
    hipError_t e = hipEventSynchronize(g_prof.ev[c][FTN_NSTAGE]);
    if (e != hipSuccess) { ftn_set_error("hipEventSynchronize: %s", hipGetErrorString(e)); return (int)e; }
    for (int s = 0; s < FTN_NSTAGE; ++s) {
      float ms = 0.f;
      e = hipEventElapsedTime(&ms, g_prof.ev[c][s], g_prof.ev[c][s + 1]);
      if (e != hipSuccess) { ftn_set_error("hipEventElapsedTime: %s", hipGetErrorString(e)); return (int)e; }
      ms_sum[s] += ms;
    }
  }
  return 0;
}

// ---------------------------------------------------------------- host side
// Upper bound of FtnDesc.total_px (grid pixels per batch row): the caller's own bound when it has one
// (ftn_selector_px_bound for the native selector, the descriptor's exact total_px for a host-built one),
// otherwise the exact worst case over any `max_groups` distinct valid periods of a window of length L
// (P_g = L + (-L mod p); periods just below L pad to almost 2L).
static int worst_px_per_row(int L, int max_groups, int px_bound) {
  if (px_bound > 0) return px_bound;
  int best[FTN_KMAX] = {0};
  for (int p = 1; p < L; ++p) {
    int v = L + (p - (L % p)) % p;
    for (int s = 0; s < max_groups; ++s)
      if (v > best[s]) { int tmp = best[s]; best[s] = v; v = tmp; }
  }
  long long w = 0;
  for (int s = 0; s < max_groups; ++s) w += best[s];
  return w > 0 ? (int)w : L;
}

// Stage C runs as separate generic pointwise launches (k_pw) when the fused kernels cannot take the shape: more
// than 16 output tiles (nbr*mid/16 + d_model/16), or a hidden chunk's weight fragments not fitting LDS twice.
static bool stagec_generic(const FtnPlan* pl) {
  if (pl->mode != 0) return false;
  const int CA = pl->nbr * pl->MP;
  const int n_ot = CA / 16 + (pl->res2 ? pl->CP / 16 : 0);
  return n_ot > 16 || pl->cfrag_per_chunk <= 0 || (size_t)pl->cfrag_per_chunk * 1024 * 2 > 160 * 1024;
}

struct WsLayout {
  size_t offA, off0, off1, off2, off3, total;
  int c0, c1;  // channel counts of buf0 / buf1
};

#define FTN_WS_HEAD 1024   // sanitised copy of the descriptor (k_guard) at the head of the workspace

static WsLayout ws_layout(const FtnPlan* pl, int B, int L, int max_groups, int px_bound) {
  WsLayout w;
  const size_t N = (size_t)B * worst_px_per_row(L, max_groups, px_bound);
  const int CA = pl->nbr * pl->MP;
  w.c0 = pl->mode == 0 ? CA : pl->CP;                 // a / a'   (mode 1: padded x, then m')
  w.c1 = pl->mode == 0 ? CA : pl->FP;                 // m / m'   (mode 1: conv1 output)
  auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
  // stage A output: one row per window position (+ pad row), shared by all period groups
  const int bpv = (pl->engine == 0 || pl->engine == 3 || pl->mode != 0) ? 4 : 6;       // fp32 / H2: 4 bytes per value, P3: 6
  w.offA = FTN_WS_HEAD;
  w.off0 = al(w.offA + ((size_t)B * L + 1) * (pl->mode == 0 ? CA : pl->CP) * bpv);
  w.off1 = al(w.off0 + N * w.c0 * bpv);
  w.off2 = al(w.off1 + N * w.c1 * bpv);               // R [N][CP]
  w.off3 = al(w.off2 + N * pl->CP * 4);               // G [N][FP] (mode 1)
  w.total = (pl->mode == 0 && !stagec_generic(pl)) ? w.off3 : al(w.off3 + N * pl->FP * 4);
  return w;
}

extern "C" size_t ftn_timesblock_workspace_bytes(const FtnPlan* plan, int B, int L, int max_groups, int px_bound) {
  if (!plan || B < 1 || L < 2 || max_groups < 1 || max_groups > FTN_KMAX || px_bound < 0) return 0;
  if ((long long)B * worst_px_per_row(L, max_groups, px_bound) > 0x7fffffffLL) return 0;   // flat pixel index is an int
  return ws_layout(plan, B, L, max_groups, px_bound).total;
}

// The kernel form of every stage of the forward (FtnForms, include/flowtimes.h): forward dispatches on exactly what this
// returns, and ftn_timesblock_forms reports it.  bfg_out (may be NULL): the split conv engine's LDS plan.
static FtnForms block_forms(const FtnPlan* pl, int L, int act_dtype, bool x_aligned, bool y_aligned, ConvBfGeom* bfg_out) {
  FtnForms f = {};
  const int C = pl->C, CP = pl->CP;
  f.mode = pl->mode; f.act = pl->act == 1 ? 1 : 0;
  f.xvec = (C % 4 == 0) && x_aligned;
  f.yvec = y_aligned;
  f.half_round = act_dtype != 0;
  if (pl->mode != 0) {
    f.stage_a_epi = -1; f.conv = FTN_FORM_CONV_FP32; f.stage_c = FTN_FORM_C_MLP; f.stage_e = FTN_FORM_E_OUT_MERGED;
    return f;
  }
  const int CA = pl->nbr * pl->MP;
  // conv engine: exact fp32 MFMA, or the bf16 matrix pipe (3 pieces = fp32-equivalent, 1 = plain bf16)
  // activation pieces: 3 = bf16x3, 2 = f16x2, 1 = plain bf16
  const int nsplit = pl->engine == 2 ? 1 : (pl->engine == 3 ? 2 : 3);
  ConvBfGeom bfg = {0, 0, 0, 0, 0, 0};
  if (pl->engine != 0) bfg = ftn_conv_bf_geom(L, pl->nbr, pl->kh, pl->kw, pl->MP, nsplit);
  if (bfg_out) *bfg_out = bfg;
  // (a kernel set whose weights do not fit the split engines' LDS plan runs on the exact fp32 MFMA kernels)
  const bool use_bf = pl->engine != 0 && bfg.NCO > 0;
  f.nsplit = use_bf ? nsplit : 0;
  f.stage_a_epi = !use_bf ? 0 : (pl->engine == 3 ? 3 : 2);
  f.conv = !use_bf ? FTN_FORM_CONV_FP32 : (bfg.fast ? FTN_FORM_CONV_BF_FAST : FTN_FORM_CONV_BF);
  f.conv_n = !use_bf ? 0 : (bfg.fast ? pl->MP / 16 : bfg.NCO);
  // stage C on the bf16 pipe too when the plan carries its fragments and the shapes fit
  const int n_ot_c = CA / 16 + (pl->res2 ? CP / 16 : 0);
  const bool mlp_bf = use_bf && pl->cfragbf_per_chunk > 0 && pl->res1 && pl->res2 && CA > 32 && CA <= 64 && CP > 32 && CP <= 64 &&
                      n_ot_c <= 8 && (size_t)pl->cfragbf_per_chunk * 3 * 1024 * 2 <= 160 * 1024;
  // the default pipeline shape (d_model 128, three kernels, mid 32): k_mlp_bf_c128
  const bool mlp_bf128 = use_bf && !mlp_bf && pl->res1 && pl->res2 && CA == 96 && CP == 128 && n_ot_c == 14 &&
                         pl->cfragbf_per_chunk == 28 &&
                         (size_t)28 * 3 * 1024 + (size_t)pl->n_hchunks * 32 * 2 * sizeof(float) <= 160 * 1024;
  // the u1 stage C of the d_model-64 shape with the FAST k_out behind it and fp32 activations: R keeps its x
  // (OutArgs.r_keeps_x); every other combination subtracts x in stage C as the reference's delta does
  const bool r_keeps_x = mlp_bf && g_mlp_u1 && g_r_keeps_x && act_dtype == 0 && (CA + 31) / 32 == 2 && (CP + 31) / 32 == 2 &&
                         n_ot_c == 7 && CA <= 48 && CP <= 64;
  // stage E on the 16-bit pipe (k_out_h): the second conv then leaves m' as activation pieces
  const bool out_h = (mlp_bf || mlp_bf128) && ftn_out_h_enabled() != 0 && pl->w_out2fb != 0 && nsplit >= 2 && act_dtype == 0 &&
                     ((CA <= 64 && CP <= 64) || (CA <= 96 && CP <= 128));
  // position-major stage C (k_mlp_pos) for the same shape: res1 / res2 once per window position, R group-summed
  const bool mlp_pos64 = mlp_bf && g_mlp_u1 && ftn_mlp_pos_enabled() != 0 && act_dtype == 0 && (CA + 31) / 32 == 2 && (CP + 31) / 32 == 2 &&
                         n_ot_c == 7 && CA == 48 && CP == 64;
  // the d_model-128 shape (f16x2): two groups per pass, one 8-wave workgroup per CU (stagec_pos.hip)
  // (its group-summed R is only understood by k_out_h at this width)
  const bool mlp_pos128 = mlp_bf128 && out_h && g_mlp_u1 && ftn_mlp_pos_enabled() != 0 && act_dtype == 0 && nsplit == 2;
  const bool mlp_pos = mlp_pos64 || mlp_pos128;
  if (mlp_bf128 && !mlp_pos128) f.stage_c = FTN_FORM_C_MLP_BF_C128;
  else if (mlp_pos) f.stage_c = mlp_pos128 ? FTN_FORM_C_MLP_POS128 : FTN_FORM_C_MLP_POS64;
  else if (mlp_bf && g_mlp_u1 && (CA + 31) / 32 == 2 && (CP + 31) / 32 == 2 && n_ot_c == 7) f.stage_c = FTN_FORM_C_MLP_BF_U1;
  else if (mlp_bf) f.stage_c = FTN_FORM_C_MLP_BF;
  else if (stagec_generic(pl)) f.stage_c = FTN_FORM_C_GENERIC;
  else f.stage_c = FTN_FORM_C_MLP;
  f.r_keeps_x = (r_keeps_x || mlp_pos) ? 1 : 0;
  f.r_summed = mlp_pos ? 1 : 0;
  f.stage_e = out_h ? FTN_FORM_E_OUT_H : (CA <= 48 && CP <= 64 ? FTN_FORM_E_OUT_FAST : FTN_FORM_E_OUT);
  return f;
}

// The one plan check, of the forwards (whose messages these are), of ftn_timesblock_forms and of the fused stage A (which answer
// a bad plan in their own words and add their own conditions).
static int plan_check(const FtnPlan* plan) {
  FTN_CHECK_ARG(plan->CP % 16 == 0 && plan->FP % 16 == 0 && plan->CP >= plan->C && plan->FP >= plan->F,
                "ftn_timesblock_forward: plan channel padding is inconsistent");
  FTN_CHECK_ARG(plan->nbr >= 1 && plan->nbr <= FTN_MAXBR, "ftn_timesblock_forward: nbr=%d", plan->nbr);
  FTN_CHECK_ARG(plan->mode == 1 || (plan->MP % 16 == 0 && plan->MP > 0), "ftn_timesblock_forward: bad MP");
  FTN_CHECK_ARG(plan->res1 || plan->CP == plan->FP, "identity res1 needs d_model == d_ff");
  FTN_CHECK_ARG(plan->res2 || plan->CP == plan->FP, "identity res2 needs d_model == d_ff");
  return 0;
}

extern "C" int ftn_timesblock_forms(const FtnPlan* plan, int B, int L, int act_dtype, int x_misalign, FtnForms* forms_out) {
  FTN_CHECK_ARG(plan && forms_out, "ftn_timesblock_forms: null pointer");
  FTN_CHECK_ARG(B >= 1 && B <= 65535 && L >= 2, "ftn_timesblock_forms: bad shape B=%d L=%d", B, L);
  FTN_CHECK_ARG(act_dtype >= 0 && act_dtype <= 2 && x_misalign >= 0 && x_misalign < 16,
                "ftn_timesblock_forms: act_dtype=%d x_misalign=%d", act_dtype, x_misalign);
  FTN_CHECK_ARG(plan_check(plan) == 0, "ftn_timesblock_forms: bad plan");
  *forms_out = block_forms(plan, L, act_dtype, x_misalign == 0, true, nullptr);
  return 0;
}

// Stage A's argument block (a = W_in1 x + b into the workspace's window rows, and the sanitised copy of desc_in at its head), for
// forward and for the fused ftn_period_finalize_stage_a.  Only the f16x2 epilogue (3) has a range to guard: any other drops the word.
static PwArgs stage_a_args(const FtnPlan* pl, const float* wb, const float* x, char* ws, const FtnDesc* desc_in, int B, int L,
                           int max_groups, int px_row, int epi, int* range_flag) {
  const int CA = pl->nbr * pl->MP;
  PwArgs pa = {};
  pa.x = x; pa.W = wb + pl->w_in1; pa.bias = wb + pl->b_in1; pa.out = (float*)(ws + FTN_WS_HEAD); pa.desc = (const FtnDesc*)ws;   // WsLayout.offA
  pa.B = B; pa.L = L; pa.C = pl->C; pa.KIN = pl->CP; pa.n_ot = CA / 16; pa.OUTC = CA;
  pa.guard_src = desc_in; pa.guard_dst = (FtnDesc*)ws; pa.guard_groups = max_groups; pa.guard_px = px_row;
  pa.range_flag = epi == 3 ? range_flag : nullptr;
  return pa;
}

static int forward(const float* x, float* y, int B, int L, const FtnPlan* pl, const float* wb, const FtnDesc* desc_in,
                   const float* wts, int max_groups, int px_bound, char* ws, hipStream_t st, const float* ln_g,
                   const float* ln_b, float ln_eps, int act_dtype, int flags, int* range_flag) {
  const WsLayout wl = ws_layout(pl, B, L, max_groups, px_bound);
  const int px_row = worst_px_per_row(L, max_groups, px_bound);
  const FtnDesc* desc = (const FtnDesc*)ws;     // sanitised copy, written by the first launch (stage A)
  float* bufA = (float*)(ws + wl.offA);
  float* buf0 = (float*)(ws + wl.off0);
  float* buf1 = (float*)(ws + wl.off1);
  float* bufR = (float*)(ws + wl.off2);
  float* bufG = (float*)(ws + wl.off3);
  const int C = pl->C, CP = pl->CP, FP = pl->FP;
  ConvBfGeom bfg = {0, 0, 0, 0, 0, 0};
  const FtnForms fm = block_forms(pl, L, act_dtype, ((uintptr_t)x & 15) == 0, ((uintptr_t)y & 15) == 0, &bfg);
  const bool xvec = fm.xvec != 0, yvec = fm.yvec != 0;
  const int act = fm.act, nsplit = fm.nsplit;
  const long long Nmax = (long long)B * px_row;
  // (tile, batch row) work items of a conv launch, estimated: every group present, a grid of ~L pixels each
  const int rows_est = (int)((long long)B * max_groups * ((L + FTN_TILE_PX - 1) / FTN_TILE_PX) < (1 << 20) ? B * max_groups * ((L + FTN_TILE_PX - 1) / FTN_TILE_PX) : 0);
  int rc = 0;
  prof_mark(0, st);
  if (pl->mode == 0) {
    const int CA = pl->nbr * pl->MP;
    const bool h2 = fm.stage_a_epi == 3;                        // the f16x2 engine
    // the split stage-C forms read m and write a' as activation pieces
    const bool c_split = fm.stage_c != FTN_FORM_C_MLP && fm.stage_c != FTN_FORM_C_GENERIC;
    // A: a = W_in1 x + b
    const PwArgs pa = stage_a_args(pl, wb, x, ws, desc_in, B, L, max_groups, px_row, fm.stage_a_epi, range_flag);
    if (!h2) range_flag = nullptr;                              // only the f16x2 engine has a range to guard
    // (FTN_FWD_STAGE_A_DONE: ftn_period_finalize_stage_a ran stage A and published the descriptor copy)
    if (!(flags & FTN_FWD_STAGE_A_DONE) && (rc = ftn_launch_stage_a(pa, nullptr, 0, act, fm.stage_a_epi, xvec, st))) return rc;
    prof_mark(1, st);
    // B: m = conv(a)
    ConvArgs ca = {};
    ConvBfArgs cb = {};
    auto conv = [&]() {
      switch (fm.conv) {
        case FTN_FORM_CONV_FP32: return ftn_launch_conv(ca, B, L, max_groups, st);
        default: return ftn_launch_conv_bf(cb, bfg, B, max_groups, nsplit, st, rows_est);   // BF / BF_FAST: as bfg says
      }
    };
    if (fm.conv == FTN_FORM_CONV_FP32) {
      ca.in = bufA; ca.bt_L = L; ca.out = buf1; ca.bias = wb + pl->b_conv1; ca.desc = desc; ca.B = B; ca.INC = CA; ca.OUTC = CA;
      ca.nbr = pl->nbr; ca.cin = pl->MP; ca.cout = pl->MP; ca.in_stride_br = pl->MP; ca.out_stride_br = pl->MP;
      for (int k = 0; k < pl->nbr; ++k) { ca.W[k] = wb + pl->w_conv1[k]; ca.kh[k] = pl->kh[k]; ca.kw[k] = pl->kw[k]; }
    } else {
      cb.range_flag = range_flag;
      cb.in = (const __bf16*)bufA; cb.bt_L = L; cb.out = buf1; cb.out_p3 = c_split ? 1 : 0; cb.bias = wb + (h2 ? pl->b_conv1s : pl->b_conv1); cb.desc = desc;
      cb.B = B; cb.INC = CA; cb.OUTC = CA; cb.nbr = pl->nbr; cb.cin = pl->MP; cb.cout = pl->MP;
      cb.in_stride_br = pl->MP / 16; cb.out_stride_br = pl->MP;
      for (int k = 0; k < pl->nbr; ++k) {
        cb.W[k] = (const __bf16*)(wb + pl->w_convbf1[k]); cb.kh[k] = pl->kh[k]; cb.kw[k] = pl->kw[k];
        cb.inv[k] = h2 ? 1.0f / pl->sc_conv1[k] : 1.0f;
      }
    }
    if ((rc = conv())) return rc;
    prof_mark(2, st);
    // C: fused pointwise chain
    switch (fm.stage_c) {
      case FTN_FORM_C_GENERIC: {
        PwArgs pg = {};
        pg.x = x; pg.desc = desc; pg.B = B; pg.L = L; pg.C = C; pg.in = buf1; pg.out = buf0; pg.R = bufR;
        rc = ftn_launch_stagec_generic(pg, pl, wb, bufG, Nmax, act, fm.stage_a_epi, xvec, st);
        break;
      }
      case FTN_FORM_C_MLP: {
        MlpArgs ma = {};
        ma.x = x; ma.m = buf1; ma.cfrag = wb + pl->w_cfrag; ma.bo = wb + pl->b_out1;
        ma.br = pl->res1 ? wb + pl->b_res1 : nullptr;
        ma.bc = wb + pl->b_c2; ma.outA = buf0; ma.outG = nullptr; ma.outR = bufR; ma.desc = desc;
        ma.B = B; ma.L = L; ma.C = C; ma.CP = CP; ma.FP = FP; ma.KM = CA; ma.AC = CA;
        ma.nKM = CA / 16; ma.nCP = pl->res1 ? CP / 16 : 0;
        ma.n_hchunks = pl->n_hchunks; ma.cfrag_per_chunk = pl->cfrag_per_chunk;
        ma.n_oa = CA / 16; ma.res2_ident = pl->res2 ? 0 : 1; ma.n_ot = ma.n_oa + (pl->res2 ? CP / 16 : 0);
        ma.outA_p3 = nsplit == 0 ? 0 : (h2 ? 2 : 1);
        rc = ftn_launch_mlp(ma, act, xvec, Nmax, st);
        break;
      }
      default: {                                                // the split-engine forms
        MlpBfArgs mb = {};
        mb.x = x; mb.m = (const __bf16*)buf1; mb.cfrag = (const __bf16*)(wb + pl->w_cfragbf);
        mb.bo = wb + (h2 ? pl->b_out1s : pl->b_out1); mb.br = wb + (h2 ? pl->b_res1s : pl->b_res1);
        mb.bc = wb + (h2 ? pl->b_c2s : pl->b_c2);
        mb.inv_o = h2 ? 1.0f / pl->sc_out1 : 1.0f; mb.sc_r = h2 ? pl->sc_res1 : 1.0f; mb.inv_r = h2 ? 1.0f / pl->sc_res1 : 1.0f;
        mb.inv_a = h2 ? 1.0f / pl->sc_a2 : 1.0f; mb.inv_r2 = h2 ? 1.0f / pl->sc_r2 : 1.0f;
        mb.r_keeps_x = fm.r_keeps_x;
        mb.range_flag = range_flag;
        mb.outA = (__bf16*)buf0; mb.outR = bufR; mb.desc = desc;
        mb.B = B; mb.L = L; mb.C = C; mb.CP = CP; mb.FP = FP; mb.KM = CA; mb.AC = CA;
        mb.nsKM = (CA + 31) / 32; mb.nsCP = (CP + 31) / 32;
        mb.n_oa = CA / 16; mb.n_ot = CA / 16 + (pl->res2 ? CP / 16 : 0); mb.n_hchunks = pl->n_hchunks; mb.per_chunk = pl->cfragbf_per_chunk;
        if (mb.per_chunk != 2 * mb.nsKM + 2 * mb.nsCP + mb.n_ot) { ftn_set_error("plan/cfragbf layout mismatch"); return -1; }
        if (fm.stage_c == FTN_FORM_C_MLP_POS64 || fm.stage_c == FTN_FORM_C_MLP_POS128) {
          MlpPosArgs mp = {};
          mp.c = mb; mp.wts = wts; mp.outRs = bufR;
          // units of 16 tail pixels per batch row: sum_g ceil(pad_g / 16) <= (sum_g pad_g + 15 G) / 16, sum_g pad_g <= px_row - L
          const int tail_row = px_row > L ? (px_row - L + 15 * max_groups) / 16 : 0;
          const long long tail_units = (long long)B * tail_row;
          const int tub = tail_units > (1 << 24) ? (1 << 24) : (int)tail_units;
          rc = fm.stage_c == FTN_FORM_C_MLP_POS128 ? ftn_launch_mlp_pos128(mp, act, xvec, tub, st)
                                                   : ftn_launch_mlp_pos64(mp, act, nsplit, xvec, tub, st);
        } else {
          rc = ftn_launch_mlp_bf(mb, fm.stage_c, act, nsplit, xvec, Nmax, st);
        }
      }
    }
    if (rc) return rc;
    prof_mark(3, st);
    // D: m' = conv(a')
    ca.in = buf0; ca.bt_L = 0; ca.out = buf1; ca.bias = wb + pl->b_conv2;
    cb.in = (const __bf16*)buf0; cb.bt_L = 0; cb.bias = wb + (h2 ? pl->b_conv2s : pl->b_conv2); cb.out_p3 = fm.stage_e == FTN_FORM_E_OUT_H ? 1 : 0;
    for (int k = 0; k < pl->nbr; ++k) {
      if (fm.conv == FTN_FORM_CONV_FP32) ca.W[k] = wb + pl->w_conv2[k];
      else { cb.W[k] = (const __bf16*)(wb + pl->w_convbf2[k]); cb.inv[k] = h2 ? 1.0f / pl->sc_conv2[k] : 1.0f; }
    }
    if ((rc = conv())) return rc;
    prof_mark(4, st);
    // E+F: y = x + sum_g w (act(W_out2 m' + b) + r)
    OutArgs oa = {};
    oa.x = x; oa.y = y; oa.m = buf1; oa.R = bufR; oa.W = wb + pl->w_out2; oa.bias = wb + pl->b_out2; oa.wts = wts;
    oa.desc = desc; oa.B = B; oa.L = L; oa.C = C; oa.CP = CP; oa.KM = CA; oa.act_dtype = act_dtype;
    oa.r_keeps_x = fm.r_keeps_x;
    oa.r_summed = fm.r_summed;
    oa.range_flag = range_flag;
    if (fm.stage_e != FTN_FORM_E_OUT) { oa.ln_g = ln_g; oa.ln_b = ln_b; oa.ln_eps = ln_eps; ln_g = nullptr; }   // fused epilogue
    switch (fm.stage_e) {
      case FTN_FORM_E_OUT_H:
        oa.mh = (const __bf16*)buf1; oa.Wf = (const __bf16*)(wb + pl->w_out2fb);
        oa.bias = wb + (h2 ? pl->b_out2s : pl->b_out2); oa.inv_out2 = h2 ? 1.0f / pl->sc_out2 : 1.0f;
        rc = ftn_launch_out_h(oa, act, nsplit, xvec && yvec, st);
        break;
      default:
        rc = ftn_launch_out(oa, act, xvec && yvec, false, fm.stage_e == FTN_FORM_E_OUT_FAST, st);
    }
    if (rc) return rc;
    prof_mark(5, st);
  } else {
    // A: zero-extended copy of x
    PwArgs pa = {};
    pa.x = x; pa.out = bufA; pa.B = B; pa.L = L; pa.C = C;
    pa.guard_src = desc_in; pa.guard_dst = (FtnDesc*)ws; pa.guard_groups = max_groups; pa.guard_px = px_row;
    if ((rc = ftn_launch_embed(pa, CP, st))) return rc;
    prof_mark(1, st);
    // B: m = conv_merged(x) (+ folded proj bias)
    ConvArgs ca = {};
    ca.in = bufA; ca.bt_L = L; ca.out = buf1; ca.bias = wb + pl->b_conv1; ca.desc = desc; ca.B = B; ca.INC = CP; ca.OUTC = FP;
    ca.nbr = 1; ca.cin = CP; ca.cout = FP; ca.in_stride_br = 0; ca.out_stride_br = 0;
    ca.W[0] = wb + pl->w_conv1[0]; ca.kh[0] = pl->kh[0]; ca.kw[0] = pl->kw[0];
    if ((rc = ftn_launch_conv(ca, B, L, max_groups, st))) return rc;
    prof_mark(2, st);
    // C: g = act(act(m) + res1(x)) -> G ; r = res2(g) - x
    MlpArgs ma = {};
    ma.x = x; ma.m = buf1; ma.cfrag = wb + pl->w_cfrag; ma.bo = nullptr;
    ma.br = pl->res1 ? wb + pl->b_res1 : nullptr;
    ma.bc = pl->res2 ? wb + pl->b_res2 : nullptr;
    ma.outA = nullptr; ma.outG = bufG; ma.outR = bufR; ma.desc = desc;
    ma.B = B; ma.L = L; ma.C = C; ma.CP = CP; ma.FP = FP; ma.KM = FP; ma.AC = 0;
    ma.nKM = 0; ma.nCP = pl->res1 ? CP / 16 : 0;
    ma.n_hchunks = pl->n_hchunks; ma.cfrag_per_chunk = pl->cfrag_per_chunk;
    ma.n_oa = 0; ma.res2_ident = pl->res2 ? 0 : 1; ma.n_ot = pl->res2 ? CP / 16 : 0;
    if (ma.n_ot > 16) { ftn_set_error("stage C needs %d output tiles (>16): d_model too large for v1", ma.n_ot); return -1; }
    if ((rc = ftn_launch_mlp(ma, act, xvec, Nmax, st))) return rc;
    prof_mark(3, st);
    // D: m' = conv_merged'(g)
    ca.in = bufG; ca.bt_L = 0; ca.out = buf0; ca.bias = wb + pl->b_conv2; ca.INC = FP; ca.OUTC = CP; ca.cin = FP; ca.cout = CP;
    ca.W[0] = wb + pl->w_conv2[0];
    if ((rc = ftn_launch_conv(ca, B, L, max_groups, st))) return rc;
    prof_mark(4, st);
    // E+F: y = x + sum_g w (act(m') + r)
    OutArgs oa = {};
    oa.x = x; oa.y = y; oa.m = buf0; oa.R = bufR; oa.W = nullptr; oa.bias = nullptr; oa.wts = wts;
    oa.desc = desc; oa.B = B; oa.L = L; oa.C = C; oa.CP = CP; oa.KM = CP; oa.act_dtype = act_dtype;
    if ((rc = ftn_launch_out(oa, act, xvec && yvec, true, false, st))) return rc;
    prof_mark(5, st);
  }
  // LayerNorm not fused above: in-place row pass over y
  if (ln_g && (rc = ftn_launch_resid_ln(x, y, y, ln_g, ln_b, ln_eps, (long long)B * L, C, st))) return rc;
  prof_mark(6, st);
  if (g_prof.on) {
    if (g_prof.sampling()) ++g_prof.calls;
    ++g_prof.seen;
  }
  return 0;
}

// rows_per_pass: 0 = the one-shot entry points (B <= 65535, one pass); >= 1 = the _rows entry points, which run stages
// A-F for rows [r0, r0 + n) pass after pass through ONE pass-sized workspace.  Rows are independent once the selection
// is fixed (every stage indexes a row's own pixels and its own w[b]), the descriptor is the same for every pass and no
// stage reads workspace bytes it has not written in the same pass, so the bits are those of a single pass.
static int forward_checked(const float* x_dev, float* y_dev, int B, int L, const FtnPlan* plan,
                           const float* wblob_dev, const FtnDesc* desc_dev, const float* weights_dev, int max_groups,
                           int px_bound, void* ws_dev, size_t ws_bytes, void* stream, const float* ln_g, const float* ln_b,
                           float ln_eps, int act_dtype, int flags, int* range_flag, int rows_per_pass) {
  FTN_CHECK_ARG(x_dev && y_dev && plan && wblob_dev && desc_dev && weights_dev && ws_dev,
                "ftn_timesblock_forward: null pointer");
  if (rows_per_pass == 0) {
    FTN_CHECK_ARG(B >= 1 && B <= 65535 && L >= 2, "ftn_timesblock_forward: bad shape B=%d L=%d", B, L);
  } else {
    FTN_CHECK_ARG(B >= 1 && L >= 2, "ftn_timesblock_forward_rows: bad shape B=%d L=%d", B, L);
    FTN_CHECK_ARG(rows_per_pass >= 1 && rows_per_pass <= 65535, "ftn_timesblock_forward_rows: rows_per_pass=%d outside [1, 65535]",
                  rows_per_pass);
  }
  const int n_pass = rows_per_pass == 0 || B <= rows_per_pass ? B : rows_per_pass;        // rows of a full pass
  FTN_CHECK_ARG(!(flags & FTN_FWD_STAGE_A_DONE) || n_pass == B,
                "ftn_timesblock_forward_rows: FTN_FWD_STAGE_A_DONE needs a single pass (B=%d rows_per_pass=%d)", B, rows_per_pass);
  FTN_CHECK_ARG(max_groups >= 1 && max_groups <= FTN_KMAX, "ftn_timesblock_forward: max_groups=%d", max_groups);
  if (plan_check(plan)) return -1;
  FTN_CHECK_ARG(px_bound >= 0, "ftn_timesblock_forward: px_bound=%d", px_bound);
  FTN_CHECK_ARG((flags & ~FTN_FWD_STAGE_A_DONE) == 0 && !((flags & FTN_FWD_STAGE_A_DONE) && plan->mode != 0),
                "ftn_timesblock_forward: flags=%d", flags);
  FTN_CHECK_ARG(act_dtype >= 0 && act_dtype <= 2 && !(act_dtype != 0 && ln_g != nullptr),
                "ftn_timesblock_forward: act_dtype=%d (the fused LayerNorm epilogue is fp32 only)", act_dtype);
  const size_t need = ftn_timesblock_workspace_bytes(plan, n_pass, L, max_groups, px_bound);
  FTN_CHECK_ARG(need > 0, "ftn_timesblock_forward: B*pixels per row exceeds 2^31 (B=%d L=%d)", n_pass, L);
  FTN_CHECK_ARG(ws_bytes >= need, "ftn_timesblock_forward: workspace %zu < %zu bytes", ws_bytes, need);
  FTN_CHECK_ARG(((uintptr_t)ws_dev & 255) == 0 && ((uintptr_t)wblob_dev & 15) == 0,
                "ftn_timesblock_forward: workspace/weights must be 256/16-byte aligned");
  // x / y are [B][L][C] fp32 and weights [B][FTN_KMAX]: a pass starts at whole rows of each (row strides L*C floats keep
  // the 16-byte alignment of x and y whenever the vector forms need it, C % 4 == 0).  range_flag is shared: every
  // writer stores 1, so the word is the OR over the passes.
  const size_t row = (size_t)L * plan->C;
  for (int r0 = 0; r0 < B; r0 += n_pass) {
    const int n = B - r0 < n_pass ? B - r0 : n_pass;
    const int rc = forward(x_dev + r0 * row, y_dev + r0 * row, n, L, plan, wblob_dev, desc_dev,
                           weights_dev + (size_t)r0 * FTN_KMAX, max_groups, px_bound, (char*)ws_dev, (hipStream_t)stream, ln_g,
                           ln_b, ln_eps, act_dtype, flags, range_flag);
    if (rc) return rc;
  }
  return 0;
}

extern "C" int ftn_timesblock_rows_per_pass(const FtnPlan* plan, int L, int max_groups, int px_bound, size_t ws_cap_bytes) {
  auto fits = [&](int n) {
    const size_t need = ftn_timesblock_workspace_bytes(plan, n, L, max_groups, px_bound);   // 0: bad shape or >= 2^31 pixels
    return need > 0 && (ws_cap_bytes == 0 || need <= ws_cap_bytes);
  };
  if (!fits(1)) return 0;
  int lo = 1, hi = 65535;                       // the workspace grows with the rows: largest n that fits
  while (lo < hi) {
    const int mid = lo + (hi - lo + 1) / 2;
    if (fits(mid)) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// S3-S5 of the selector and stage A of the block in ONE launch (k_finalize_pw, stage_a.hip): see flowtimes.h
extern "C" int ftn_period_finalize_stage_a(const double* psum_dev, int nparts, int Btotal, const float* med_dev, int B,
                                           int L, int k_periods, int pmax, int min_period_threshold, int act_dtype,
                                           int max_unique, double log_base, FtnDesc* desc_dev, float* amps_dev,
                                           float* weights_dev, const float* x_dev, const FtnPlan* plan,
                                           const float* wblob_dev, int max_groups, int px_bound, void* ws_dev,
                                           size_t ws_bytes, void* stream, int* range_flag_dev, const FtnExchange* xch) {
  // psum_dev == NULL: stage A only;  x_dev == NULL: finalize + descriptor copy only (stage A is in the workspace)
  const bool do_fin = psum_dev != nullptr || xch != nullptr, do_a = x_dev != nullptr;
  const char* who = "ftn_period_finalize_stage_a";
  // (this entry has always looked at the exchange first; ftn_finalize_check looks again, where ftn_period_finalize does)
  FTN_CHECK_ARG(xch == nullptr || ftn_xch_ok(xch, L / 2 + 1), "%s: bad exchange (world / rank / seq / mode / F_cap)", who);
  FTN_CHECK_ARG(do_fin || do_a, "ftn_period_finalize_stage_a: nothing to do (psum and x both null)");
  FTN_CHECK_ARG(plan && wblob_dev && ws_dev, "ftn_period_finalize_stage_a: null pointer");
  int rc;
  if (do_fin && (rc = ftn_finalize_check(who, psum_dev, nparts, Btotal, med_dev, B, L, desc_dev, amps_dev, weights_dev, xch))) return rc;
  // (the row limit belongs to stage A, whose workspace holds all B rows; the finalize-only part has none)
  FTN_CHECK_ARG(B >= 1 && (B <= 65535 || !do_a) && L >= 2, "ftn_period_finalize_stage_a: bad shape");
  FTN_CHECK_ARG(k_periods <= FTN_KMAX && act_dtype >= 0 && act_dtype <= 2, "ftn_period_finalize_stage_a: k=%d act_dtype=%d", k_periods, act_dtype);
  FTN_CHECK_ARG(plan_check(plan) == 0 && plan->mode == 0, "ftn_period_finalize_stage_a: bottleneck blocks only");
  FTN_CHECK_ARG(max_groups >= 1 && max_groups <= FTN_KMAX && px_bound >= 0, "ftn_period_finalize_stage_a: bounds");
  const size_t need = ftn_timesblock_workspace_bytes(plan, B, L, max_groups, px_bound);
  FTN_CHECK_ARG(need > 0 && ws_bytes >= need && ((uintptr_t)ws_dev & 255) == 0 && ((uintptr_t)wblob_dev & 15) == 0,
                "ftn_period_finalize_stage_a: workspace %zu < %zu bytes or misaligned", ws_bytes, need);
  FinalizeArgs fa;
  if ((rc = ftn_finalize_args(who, psum_dev, nparts, Btotal, med_dev, B, L, k_periods, pmax, min_period_threshold, act_dtype,
                              max_unique, log_base, desc_dev, amps_dev, weights_dev, xch, &fa)))
    return rc;
  size_t stamp_cap;
  fa.dbg = ftn_stamp_buf(8, &stamp_cap);
  if (stamp_cap < 8) fa.dbg = nullptr;
  const FtnForms fm = block_forms(plan, L, act_dtype, x_dev != nullptr && ((uintptr_t)x_dev & 15) == 0, true, nullptr);
  const PwArgs pa = stage_a_args(plan, wblob_dev, x_dev, (char*)ws_dev, desc_dev, B, L, max_groups,
                                 worst_px_per_row(L, max_groups, px_bound), fm.stage_a_epi, range_flag_dev);
  const int part = do_fin && do_a ? 0 : (do_a ? 1 : 2);
  return ftn_launch_stage_a(pa, &fa, part, fm.act, fm.stage_a_epi, fm.xvec != 0, (hipStream_t)stream);
}

extern "C" int ftn_timesblock_forward(const float* x_dev, float* y_dev, int B, int L, const FtnPlan* plan,
                                      const float* wblob_dev, const FtnDesc* desc_dev, const float* weights_dev,
                                      int max_groups, int px_bound, int act_dtype, int flags, void* ws_dev,
                                      size_t ws_bytes, void* stream, int* range_flag_dev) {
  return forward_checked(x_dev, y_dev, B, L, plan, wblob_dev, desc_dev, weights_dev, max_groups, px_bound, ws_dev, ws_bytes,
                         stream, nullptr, nullptr, 0.f, act_dtype, flags, range_flag_dev, 0);
}

extern "C" int ftn_timesblock_forward_rows(const float* x_dev, float* y_dev, int B, int L, const FtnPlan* plan,
                                           const float* wblob_dev, const FtnDesc* desc_dev, const float* weights_dev,
                                           int max_groups, int px_bound, int act_dtype, int flags, void* ws_dev,
                                           size_t ws_bytes, void* stream, int* range_flag_dev, int rows_per_pass) {
  FTN_CHECK_ARG(rows_per_pass != 0, "ftn_timesblock_forward_rows: rows_per_pass=0 outside [1, 65535]");
  return forward_checked(x_dev, y_dev, B, L, plan, wblob_dev, desc_dev, weights_dev, max_groups, px_bound, ws_dev, ws_bytes,
                         stream, nullptr, nullptr, 0.f, act_dtype, flags, range_flag_dev, rows_per_pass);
}

extern "C" int ftn_timesblock_forward_norm(const float* x_dev, float* y_dev, int B, int L, const FtnPlan* plan,
                                           const float* wblob_dev, const FtnDesc* desc_dev, const float* weights_dev,
                                           int max_groups, int px_bound, int flags, const float* ln_gamma_dev,
                                           const float* ln_beta_dev, float ln_eps, void* ws_dev, size_t ws_bytes,
                                           void* stream, int* range_flag_dev) {
  FTN_CHECK_ARG(ln_gamma_dev && ln_beta_dev && ln_eps >= 0.f, "ftn_timesblock_forward_norm: LayerNorm parameters");
  return forward_checked(x_dev, y_dev, B, L, plan, wblob_dev, desc_dev, weights_dev, max_groups, px_bound, ws_dev,
                         ws_bytes, stream, ln_gamma_dev, ln_beta_dev, ln_eps, 0, flags, range_flag_dev, 0);
}

extern "C" int ftn_timesblock_forward_norm_rows(const float* x_dev, float* y_dev, int B, int L, const FtnPlan* plan,
                                                const float* wblob_dev, const FtnDesc* desc_dev, const float* weights_dev,
                                                int max_groups, int px_bound, int flags, const float* ln_gamma_dev,
                                                const float* ln_beta_dev, float ln_eps, void* ws_dev, size_t ws_bytes,
                                                void* stream, int* range_flag_dev, int rows_per_pass) {
  FTN_CHECK_ARG(ln_gamma_dev && ln_beta_dev && ln_eps >= 0.f, "ftn_timesblock_forward_norm_rows: LayerNorm parameters");
  FTN_CHECK_ARG(rows_per_pass != 0, "ftn_timesblock_forward_norm_rows: rows_per_pass=0 outside [1, 65535]");
  return forward_checked(x_dev, y_dev, B, L, plan, wblob_dev, desc_dev, weights_dev, max_groups, px_bound, ws_dev,
                         ws_bytes, stream, ln_gamma_dev, ln_beta_dev, ln_eps, 0, flags, range_flag_dev, rows_per_pass);
}

extern "C" int ftn_residual_layernorm(const float* x_dev, const float* new_dev, float* out_dev, long long rows, int C,
                                      const float* ln_gamma_dev, const float* ln_beta_dev, float ln_eps,
                                      void* stream) {
  FTN_CHECK_ARG(x_dev && new_dev && out_dev && ln_gamma_dev && ln_beta_dev, "ftn_residual_layernorm: null pointer");
  FTN_CHECK_ARG(rows >= 1 && rows <= 0x7fffffffLL * 4 && C >= 1, "ftn_residual_layernorm: rows=%lld C=%d", rows, C);
  return ftn_launch_resid_ln(x_dev, new_dev, out_dev, ln_gamma_dev, ln_beta_dev, ln_eps, rows, C, (hipStream_t)stream);
}
