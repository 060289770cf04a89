// The C entry points of the model shell (include/flowtimes.h): host code only, no kernel.  Every exported function
// forwards to the one body of its operation with its own name (every message starts with it), its width (ShellWidth,
// ftn_shell.h: the entry names it, d_model does not pick it) and, for the embedding, its norm.  A body checks the
// arguments, fills the argument block and hands it to the launch of the width's kernel unit (shell.hip,
// shell_wide.hip, timeproj.hip), which chooses the form.
#include "ftn_common.h"
#include "ftn_shell.h"

#define FTN_CHECK_D_MODEL(who, w, D) \
  FTN_CHECK_ARG((w).d_ok(D), "%s: d_model=%d must be a multiple of 4, %s", who, D, (w).range)

// --------------------------------------------------------------------------------------------------------- heads
static int head_form_entry(const char* who, const ShellWidth& w, int N, int D, long long tail_bs, long long late_bs,
                           int misalign_or) {
  FTN_CHECK_ARG(N >= 1 && w.d_ok(D) && misalign_ok(misalign_or), "%s: N=%d d_model=%d misalign=%d", who, N, D, misalign_or);
  return (w.wide ? head_wide_form : head_form)(N, D, tail_bs, late_bs, (unsigned)misalign_or);
}

static int head_entry(const char* who, const ShellWidth& w, const float* hidden, long long rows, int S, int D, int N,
                      const float* wmu, const float* bmu, const float* wsg, const float* bsg, const float* tail,
                      long long tail_bs, int hist, const float* late, long long late_bs, const float* floorv,
                      float floor_s, float* rate, float* disp, int* bad, void* stream) {
  FTN_CHECK_ARG(hidden && wmu && bmu && wsg && bsg && tail && rate && disp && bad, "%s: null pointer", who);
  FTN_CHECK_ARG(rows >= 1 && S >= 1 && rows % S == 0 && N >= 1 && hist >= 1 && hist <= S,
                "%s: rows=%lld S=%d N=%d hist=%d", who, rows, S, N, hist);
  FTN_CHECK_D_MODEL(who, w, D);
  FTN_CHECK_ARG((((uintptr_t)hidden | (uintptr_t)wmu | (uintptr_t)wsg) & 15) == 0,
                "%s: hidden and the head weights must be 16-byte aligned", who);
  if (w.align4)                                                 // wide only, deliberately (ShellWidth)
    FTN_CHECK_ARG((((uintptr_t)bmu | (uintptr_t)bsg | (uintptr_t)tail | (uintptr_t)late | (uintptr_t)floorv |
                    (uintptr_t)rate | (uintptr_t)disp | (uintptr_t)bad) & 3) == 0,
                  "%s: every operand must be 4-byte aligned", who);
  HeadArgs a;
  a.hidden = hidden; a.wmu = wmu; a.bmu = bmu; a.wsg = wsg; a.bsg = bsg;
  a.tail = tail; a.late = late; a.floorv = floorv; a.rate = rate; a.disp = disp; a.bad = bad;
  a.sig_mu = a.sig_sg = nullptr;
  a.rows = rows; a.tail_bs = tail_bs; a.late_bs = late_bs;
  a.S = S; a.D = D; a.N = N; a.hist = hist; a.floor_s = floor_s;
  return (w.wide ? head_wide_launch : head_launch)(a, (hipStream_t)stream);
}

// ----------------------------------------------------------------------------------------------- value embedding
static int embed_form_entry(const char* who, const ShellWidth& w, int N, int D, long long x_bs, int x_misalign,
                            int w_misalign) {
  FTN_CHECK_ARG(N >= 1 && w.d_ok(D) && misalign_ok(x_misalign) && misalign_ok(w_misalign),
                "%s: N=%d d_model=%d misalign=%d/%d", who, N, D, x_misalign, w_misalign);
  return (w.wide ? embed_wide_form : embed_form)(N, D, x_bs, (unsigned)(x_misalign | w_misalign));
}

// norm: FTN_NORM_LAYER takes both of gamma / beta or neither (no norm), FTN_NORM_RMS needs both
static int check_norm(const char* who, int norm, const float* gamma, const float* beta) {
  if (norm == FTN_NORM_RMS) FTN_CHECK_ARG(gamma && beta, "%s: the RMS norm needs gamma and beta", who);
  FTN_CHECK_ARG((gamma == nullptr) == (beta == nullptr), "%s: LayerNorm needs both gamma and beta", who);
  return 0;
}

// The full embedding (out_bs null: rows of a [B][L][D] result), and the GEMM alone into rows of a larger buffer
// (ftn_embed*_rows_strided: out_bs given; no add, no norm): row (b, l) of x W^T lands at out + b * out_bs + l * D.
// Same kernels, same form selection and same K order, so such a row is bit-identical to what the full call computes
// for it before its epilogue.  The recursive forecaster (forecast.py) appends each step's B new rows (L = 1) to its
// ring of embedded rows with it.
static int embed_entry(const char* who, const ShellWidth& w, int norm, const float* x, long long x_bs, int B, int L,
                       int N, const float* W, int D, const float* add, long long add_bs, const float* gamma,
                       const float* beta, float eps, float* out, const long long* out_bs, void* stream) {
  FTN_CHECK_ARG(x && W && out, "%s: null pointer", who);
  FTN_CHECK_ARG(B >= 1 && L >= 1 && N >= 1, "%s: bad shape B=%d L=%d N=%d", who, B, L, N);
  FTN_CHECK_D_MODEL(who, w, D);
  if (w.rows_fit_grid)                                          // wide only, deliberately (ShellWidth)
    FTN_CHECK_ARG((long long)B * L <= 0x7fffffffLL, "%s: B=%d L=%d exceed the launch grid", who, B, L);
  if (out_bs)
    FTN_CHECK_ARG(B == 1 || *out_bs >= (long long)L * D, "%s: out_bstride=%lld < L*D=%lld", who, *out_bs, (long long)L * D);
  if (check_norm(who, norm, gamma, beta)) return -1;
  if (w.align4)                                                 // wide only, deliberately (ShellWidth)
    FTN_CHECK_ARG((((uintptr_t)x | (uintptr_t)W) & 3) == 0, "%s: x and W must be 4-byte aligned", who);
  if (out_bs)
    FTN_CHECK_ARG(((uintptr_t)out & 15) == 0 && *out_bs % 4 == 0,
                  "%s: out must be 16-byte aligned, out_bstride a multiple of 4", who);
  else
    FTN_CHECK_ARG((((uintptr_t)out | (uintptr_t)add | (uintptr_t)gamma | (uintptr_t)beta) & 15) == 0 && add_bs % 4 == 0,
                  "%s: out / add / LayerNorm parameters must be 16-byte aligned", who);
  EmbedArgs a;
  a.x = x; a.W = W; a.add = add; a.ln_g = gamma; a.ln_b = beta;
  a.out = out; a.x_bs = x_bs; a.add_bs = add_bs; a.out_bs = out_bs ? *out_bs : (long long)L * D;
  a.B = B; a.L = L; a.N = N; a.D = D; a.ln_eps = eps; a.norm = gamma ? norm : FTN_NORM_NONE;
  return (w.wide ? embed_wide_launch : embed_launch)(a, (hipStream_t)stream);
}

static int ring_entry(const char* who, const ShellWidth& w, int norm, const float* V, int B, int L, int D, int head,
                      const float* add, long long add_bs, const float* gamma, const float* beta, float eps, float* out,
                      void* stream) {
  FTN_CHECK_ARG(V && out, "%s: null pointer", who);
  FTN_CHECK_ARG(B >= 1 && L >= 1, "%s: bad shape B=%d L=%d", who, B, L);
  FTN_CHECK_D_MODEL(who, w, D);
  if (w.rows_fit_grid)                                          // wide only, deliberately (ShellWidth)
    FTN_CHECK_ARG((long long)B * L <= 0x7fffffffLL, "%s: B=%d L=%d exceed the launch grid", who, B, L);
  FTN_CHECK_ARG(head >= 0 && head < L, "%s: head=%d outside [0, L=%d)", who, head, L);
  if (check_norm(who, norm, gamma, beta)) return -1;
  FTN_CHECK_ARG((((uintptr_t)V | (uintptr_t)out | (uintptr_t)add | (uintptr_t)gamma | (uintptr_t)beta) & 15) == 0 &&
                    add_bs % 4 == 0 && add_bs >= 0,
                "%s: V / out / add / LayerNorm parameters must be 16-byte aligned", who);
  RingArgs a;
  a.V = V; a.add = add; a.ln_g = gamma; a.ln_b = beta; a.out = out;
  a.add_bs = add_bs; a.B = B; a.L = L; a.D = D; a.head = head; a.ln_eps = eps;
  a.norm = gamma ? norm : FTN_NORM_NONE;
  return (w.wide ? ring_wide_launch : ring_launch)(a, (hipStream_t)stream);
}

// ----------------------------------------------------------------------------------------------- time projection
static int timeproj_form_entry(const char* who, const ShellWidth& w, int L, int S, int D, int wt_misalign) {
  FTN_CHECK_ARG(L >= 1 && S >= 1 && w.d_ok(D) && misalign_ok(wt_misalign), "%s: L=%d S=%d d_model=%d misalign=%d", who,
                L, S, D, wt_misalign);
  return timeproj_form(L, S, (unsigned)wt_misalign);
}

// mapped (the _rows entries): seq is an item store [n_items][L][D] read through rows [B]; else rows is null.
static int timeproj_entry(const char* who, const ShellWidth& w, bool mapped, const float* seq, long long n_items,
                          const long long* rows, int B, int L, int D, const float* wt, const float* bt, int S,
                          float* hidden, void* stream) {
  FTN_CHECK_ARG(seq && wt && bt && hidden && (rows || !mapped), "%s: null pointer", who);
  FTN_CHECK_ARG(B >= 1 && L >= 1 && S >= 1, "%s: bad shape B=%d L=%d S=%d", who, B, L, S);
  FTN_CHECK_ARG(n_items >= 1, "%s: n_items=%lld must be >= 1", who, n_items);
  FTN_CHECK_ARG(((uintptr_t)rows & 7) == 0, "%s: rows must be 8-byte aligned", who);
  FTN_CHECK_D_MODEL(who, w, D);
  FTN_CHECK_ARG((((uintptr_t)seq | (uintptr_t)hidden) & 15) == 0, "%s: seq and hidden must be 16-byte aligned", who);
  FTN_CHECK_ARG((((uintptr_t)wt | (uintptr_t)bt) & 3) == 0, "%s: W_t and b_t must be 4-byte aligned", who);
  FTN_CHECK_ARG((long long)B * ((D + 63) / 64) <= 0x7fffffffLL && (S + 15) / 16 <= 65535,
                "%s: B=%d S=%d exceed the launch grid", who, B, S);
  TimeProjArgs a;
  a.seq = seq; a.rows = rows; a.n_items = n_items; a.wt = wt; a.bt = bt; a.hid = hidden;
  a.B = B; a.L = L; a.D = D; a.S = S;
  return timeproj_launch(a, w, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------ the exported functions
// One forward each (include/flowtimes.h documents the arguments): the entry adds its name, its width and its norm.
#define HEAD_ARGS hidden, rows, S, D, N, wmu, bmu, wsg, bsg, tail, tail_bs, hist, late, late_bs, floorv, floor_s, rate, disp, bad, stream
#define EMBED_ARGS x, x_bs, B, L, N, W, D, add, add_bs, gamma, beta, eps, out, nullptr, stream
#define ROWS_ARGS FTN_NORM_LAYER, x, x_bs, B, L, N, W, D, nullptr, 0, nullptr, nullptr, 0.f, out, &out_bs, stream
#define RING_ARGS V, B, L, D, head, add, add_bs, gamma, beta, eps, out, stream
extern "C" {
int ftn_head_forward(const float* hidden, long long rows, int S, int D, int N, const float* wmu, const float* bmu,
                     const float* wsg, const float* bsg, const float* tail, long long tail_bs, int hist,
                     const float* late, long long late_bs, const float* floorv, float floor_s, float* rate,
                     float* disp, int* bad, void* stream) {
  return head_entry("ftn_head_forward", kShellNarrow, HEAD_ARGS);
}
int ftn_head_wide_forward(const float* hidden, long long rows, int S, int D, int N, const float* wmu, const float* bmu,
                          const float* wsg, const float* bsg, const float* tail, long long tail_bs, int hist,
                          const float* late, long long late_bs, const float* floorv, float floor_s, float* rate,
                          float* disp, int* bad, void* stream) {
  return head_entry("ftn_head_wide_forward", kShellWide, HEAD_ARGS);
}
int ftn_head_form(int N, int D, long long tail_bs, long long late_bs, int misalign_or) {
  return head_form_entry("ftn_head_form", kShellNarrow, N, D, tail_bs, late_bs, misalign_or);
}
int ftn_head_wide_form(int N, int D, long long tail_bs, long long late_bs, int misalign_or) {
  return head_form_entry("ftn_head_wide_form", kShellWide, N, D, tail_bs, late_bs, misalign_or);
}

int ftn_embed_forward(const float* x, long long x_bs, int B, int L, int N, const float* W, int D, const float* add,
                      long long add_bs, const float* gamma, const float* beta, float eps, float* out, void* stream) {
  return embed_entry("ftn_embed_forward", kShellNarrow, FTN_NORM_LAYER, EMBED_ARGS);
}
int ftn_embed_forward_rms(const float* x, long long x_bs, int B, int L, int N, const float* W, int D, const float* add,
                          long long add_bs, const float* gamma, const float* beta, float eps, float* out, void* stream) {
  return embed_entry("ftn_embed_forward_rms", kShellNarrow, FTN_NORM_RMS, EMBED_ARGS);
}
int ftn_embed_wide_forward(const float* x, long long x_bs, int B, int L, int N, const float* W, int D, const float* add,
                           long long add_bs, const float* gamma, const float* beta, float eps, float* out, void* stream) {
  return embed_entry("ftn_embed_wide_forward", kShellWide, FTN_NORM_LAYER, EMBED_ARGS);
}
int ftn_embed_wide_forward_rms(const float* x, long long x_bs, int B, int L, int N, const float* W, int D,
                               const float* add, long long add_bs, const float* gamma, const float* beta, float eps,
                               float* out, void* stream) {
  return embed_entry("ftn_embed_wide_forward_rms", kShellWide, FTN_NORM_RMS, EMBED_ARGS);
}
int ftn_embed_rows_strided(const float* x, long long x_bs, int B, int L, int N, const float* W, int D, float* out,
                           long long out_bs, void* stream) {
  return embed_entry("ftn_embed_rows_strided", kShellNarrow, ROWS_ARGS);
}
int ftn_embed_wide_rows_strided(const float* x, long long x_bs, int B, int L, int N, const float* W, int D, float* out,
                                long long out_bs, void* stream) {
  return embed_entry("ftn_embed_wide_rows_strided", kShellWide, ROWS_ARGS);
}
int ftn_embed_ring(const float* V, int B, int L, int D, int head, const float* add, long long add_bs,
                   const float* gamma, const float* beta, float eps, float* out, void* stream) {
  return ring_entry("ftn_embed_ring", kShellNarrow, FTN_NORM_LAYER, RING_ARGS);
}
int ftn_embed_ring_rms(const float* V, int B, int L, int D, int head, const float* add, long long add_bs,
                       const float* gamma, const float* beta, float eps, float* out, void* stream) {
  return ring_entry("ftn_embed_ring_rms", kShellNarrow, FTN_NORM_RMS, RING_ARGS);
}
int ftn_embed_wide_ring(const float* V, int B, int L, int D, int head, const float* add, long long add_bs,
                        const float* gamma, const float* beta, float eps, float* out, void* stream) {
  return ring_entry("ftn_embed_wide_ring", kShellWide, FTN_NORM_LAYER, RING_ARGS);
}
int ftn_embed_wide_ring_rms(const float* V, int B, int L, int D, int head, const float* add, long long add_bs,
                            const float* gamma, const float* beta, float eps, float* out, void* stream) {
  return ring_entry("ftn_embed_wide_ring_rms", kShellWide, FTN_NORM_RMS, RING_ARGS);
}
int ftn_embed_form(int N, int D, long long x_bs, int x_misalign, int w_misalign) {
  return embed_form_entry("ftn_embed_form", kShellNarrow, N, D, x_bs, x_misalign, w_misalign);
}
int ftn_embed_wide_form(int N, int D, long long x_bs, int x_misalign, int w_misalign) {
  return embed_form_entry("ftn_embed_wide_form", kShellWide, N, D, x_bs, x_misalign, w_misalign);
}

int ftn_timeproj_forward(const float* seq, int B, int L, int D, const float* wt, const float* bt, int S, float* hidden,
                         void* stream) {
  return timeproj_entry("ftn_timeproj_forward", kShellNarrow, false, seq, 1, nullptr, B, L, D, wt, bt, S, hidden,
                        stream);
}
int ftn_timeproj_forward_rows(const float* seq, long long n_items, const long long* rows, int B, int L, int D,
                              const float* wt, const float* bt, int S, float* hidden, void* stream) {
  return timeproj_entry("ftn_timeproj_forward_rows", kShellNarrow, true, seq, n_items, rows, B, L, D, wt, bt, S, hidden,
                        stream);
}
int ftn_timeproj_wide_forward(const float* seq, int B, int L, int D, const float* wt, const float* bt, int S,
                              float* hidden, void* stream) {
  return timeproj_entry("ftn_timeproj_wide_forward", kShellWide, false, seq, 1, nullptr, B, L, D, wt, bt, S, hidden,
                        stream);
}
int ftn_timeproj_wide_forward_rows(const float* seq, long long n_items, const long long* rows, int B, int L, int D,
                                   const float* wt, const float* bt, int S, float* hidden, void* stream) {
  return timeproj_entry("ftn_timeproj_wide_forward_rows", kShellWide, true, seq, n_items, rows, B, L, D, wt, bt, S,
                        hidden, stream);
}
int ftn_timeproj_form(int L, int S, int D, int wt_misalign) {
  return timeproj_form_entry("ftn_timeproj_form", kShellNarrow, L, S, D, wt_misalign);
}
int ftn_timeproj_wide_form(int L, int S, int D, int wt_misalign) {
  return timeproj_form_entry("ftn_timeproj_wide_form", kShellWide, L, S, D, wt_misalign);
}
}
