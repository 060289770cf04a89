/* flowtimes.h — C ABI of libflowtimes_hip.so (MI355X / gfx950).
 *
 * The reference (ShinDongWoon/Flow-TimesNet) is pure Python/PyTorch and has no
 * FFI of its own (SURVEY.md finding 1); this ABI is therefore build-defined and
 * each entry point cites the reference code it replaces
 * (paths relative to src/timesnet_forecast/models/timesnet.py).
 *
 * Conventions
 *  - every pointer marked "dev" is a device pointer owned by the caller
 *    (PyTorch tensors); nothing is allocated or freed behind the caller's back;
 *  - every call only ENQUEUES work on `stream` (a hipStream_t passed as void*)
 *    and never synchronises, so a sequence of calls can be captured in a hipGraph;
 *  - return value: 0 = ok, <0 = bad argument (see ftn_last_error), >0 = hipError_t;
 *  - all tensors are fp32, contiguous, C (channel) fastest: x[B][L][C].
 */
#ifndef FLOWTIMES_H
#define FLOWTIMES_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FTN_ABI_VERSION 14
#define FTN_KMAX 16      /* max period candidates / groups per block call        */
#define FTN_MAXBR 8      /* max kernels in kernel_set                             */

/* Device-side period descriptor: what PeriodGrouper.group() returns on the host
 * in the reference (PeriodGroupResult, :275-283) plus the tiling the conv kernels
 * use.  Written by ftn_period_finalize (device) or built on the host by
 * ftn_desc_from_periods and copied up; read by every ftn_timesblock_* kernel, so
 * the host never has to synchronise to learn data-dependent shapes. */
typedef struct FtnDesc {
  int32_t n_sel;                    /* K': periods kept by the selector (:153)           */
  int32_t n_groups;                 /* G: distinct valid periods (:551)                  */
  int32_t total_px;                 /* sum_g (L + pad_g): grid pixels per batch row      */
  int32_t tiles_per_row;            /* sum_g ntx*nty: conv tiles per batch row           */
  int32_t sel_freq[FTN_KMAX];       /* rFFT bin of each kept candidate (:156)            */
  int32_t sel_period[FTN_KMAX];     /* period of each kept candidate, score order (:157) */
  int32_t sel_group[FTN_KMAX];      /* mapping[K] -> group id or -1 (:460-477)           */
  int32_t g_period[FTN_KMAX];       /* group periods, ascending (:453-458)               */
  int32_t g_pad[FTN_KMAX];          /* (-L) mod p (:531)                                 */
  int32_t g_cycles[FTN_KMAX];       /* (L+pad)/p (:533)                                  */
  int32_t g_px_off[FTN_KMAX + 1];   /* prefix sums of (L+pad_g)                          */
  int32_t g_tw[FTN_KMAX];           /* conv tile width  (phase axis)                     */
  int32_t g_th[FTN_KMAX];           /* conv tile height (cycle axis)                     */
  int32_t g_ntx[FTN_KMAX];
  int32_t g_nty[FTN_KMAX];
  int32_t g_tile_off[FTN_KMAX + 1]; /* prefix sums of ntx*nty                            */
} FtnDesc;

/* Host-side description of one TimesBlock's (folded, packed) inception weights.
 * Filled by ftn_inception_pack_weights (host); offsets are in floats
 * into the weight blob.  Replaces nn.Sequential(InceptionBlock, act,
 * InceptionBlock) (:744-762) for inference. */
typedef struct FtnPlan {
  int32_t C, CP;          /* d_model, padded to 16                                          */
  int32_t F, FP;          /* d_ff, padded to 16                                             */
  int32_t mode;           /* 0: bottleneck branches (:581-590); 1: single conv (:575-580)   */
  int32_t act;            /* 0: GELU(erf) (:643), 1: ReLU (:641)                            */
  int32_t nbr;            /* conv branches: mode 0 = len(kernel_set); mode 1 = 1 (merged)   */
  int32_t MP;             /* mode 0: mid channels per branch padded to 16                   */
  int32_t kh[FTN_MAXBR], kw[FTN_MAXBR];
  int32_t res1, res2;     /* 1 = res_proj conv present (:634-635), 0 = identity (:637)      */
  /* block 1 (d_model -> d_ff) */
  int64_t w_in1, b_in1;   /* mode 0: [nbr*MP][CP] 1x1 in->mid, bias                         */
  int64_t w_conv1[FTN_MAXBR]; /* [taps][cin/16][cout/16][16][16]                            */
  int64_t b_conv1;        /* mode 0: [nbr*MP]; mode 1: [FP] (proj folded)                   */
  int64_t w_out1, b_out1; /* mode 0: folded proj.branch[-1]: [FP][nbr*MP], [FP]             */
  int64_t w_res1, b_res1; /* [FP][CP], [FP]                                                 */
  /* block 2 (d_ff -> d_model) */
  int64_t w_in2, b_in2;   /* mode 0: [nbr*MP][FP]                                           */
  int64_t w_conv2[FTN_MAXBR];
  int64_t b_conv2;        /* mode 0: [nbr*MP]; mode 1: [CP]                                 */
  int64_t w_out2, b_out2; /* mode 0: [CP][nbr*MP], [CP]                                     */
  int64_t w_res2, b_res2; /* [CP][FP], [CP]                                                 */
  /* stage-C output projection = rows [w_in2 ; w_res2] stacked: [(nbr*MP + CP)][FP]        */
  int64_t w_c2, b_c2;
  /* the same stage-C matrices as lane-linear MFMA fragments, grouped per 32-channel
   * hidden chunk: [chunk][ w_out1: 2 tiles x KM/16 | w_res1: 2 x CP/16 | w_c2: 2 x n_ot ][lane][4]
   * (rows/cols beyond FP are zero fragments) */
  int64_t w_cfrag;
  int32_t cfrag_per_chunk;  /* fragments (of 256 floats) per hidden chunk */
  int32_t n_hchunks;        /* ceil(FP / 32)                               */
  /* bf16x3 conv engine (mode 0 only): per branch the k x k weights as three bf16 pieces in
   * K=32 MFMA fragments, [cin/16][cout/16][slab = tap pair][piece][lane][8] (offsets in
   * floats; the data are bf16).  engine: 0 = exact fp32 MFMA, 1 = bf16x3 split, 2 = plain bf16,
   * 3 = f16x2 split (below) */
  int64_t w_convbf1[FTN_MAXBR];
  int64_t w_convbf2[FTN_MAXBR];
  int32_t engine;
  /* bf16x3 stage-C fragments per 32-channel hidden chunk (3 pieces x 1 KiB each; only when both
   * res_proj convs exist): [chunk][w_out1 2 x ceil(KM/32) | w_res1 2 x ceil(CP/32) | w_c n_ot][piece] */
  int32_t cfragbf_per_chunk;
  int64_t w_cfragbf;
  /* f16x2 engine (engine 3; mode 0 only): w_convbf1/2 and w_cfragbf then hold THREE fp16 pieces per weight
   * fragment - A1 = fp16(W~), A2 = fp16(A1 2^-11), A3 = fp16(W~ - A1) of the prescaled matrix W~ = sc W with
   * sc a power of two (per conv branch, per stage-C matrix) - and activations travel as two fp16 pieces
   * (hi, (x - hi) 2^11).  The kernels start their accumulators from biases prescaled by the same sc (offsets
   * below) and multiply by 1/sc when they leave the matrix pipe. */
  int64_t b_conv1s, b_conv2s, b_out1s, b_res1s, b_c2s;
  float sc_conv1[FTN_MAXBR], sc_conv2[FTN_MAXBR];
  float sc_out1, sc_res1, sc_a2, sc_r2;   /* W_out1, W_res1, W_in2 rows of w_c2, W_res2 rows of w_c2 */
  /* split engines, stage E on the 16-bit matrix pipe (the shapes that carry w_cfragbf): w_out2 as K=32 fragments of
   * three pieces, [CP/16 row tiles][ceil(nbr*MP/32) slabs][piece][lane][8] (0 = absent); f16x2: of sc_out2 w_out2,
   * with b_out2s = sc_out2 b_out2 */
  int64_t w_out2fb, b_out2s;
  float sc_out2;
  int32_t reserved0;
  int64_t total_floats;
} FtnPlan;

int ftn_abi_version(void);
const char* ftn_last_error(void);

/* ---- weight folding + packing (host only): replaces nn.Sequential(InceptionBlock, act, InceptionBlock) ---- */
/* The reference state_dict tensors of ONE InceptionBlock (:622-637) as raw host pointers (fp32, contiguous):
 * paths.{j}.branch.{i}.{weight,bias} - bottleneck branches (:581-590): i = 0 [mid][in][1][1], 1 [mid][mid][kh][kw],
 * 2 [out][mid][1][1]; single-conv branches (ratio 1, :575-580): only i = 0, [out][in][kh][kw] - proj.{weight,bias}
 * [out][out*nk][1][1], res_proj.{weight,bias} [out][in][1][1] or NULL when in == out (nn.Identity, :637). */
typedef struct FtnInceptionBlockWeights {
  const float* branch_w[FTN_MAXBR][3];
  const float* branch_b[FTN_MAXBR][3];
  const float* proj_w;
  const float* proj_b;
  const float* res_w;
  const float* res_b;
} FtnInceptionBlockWeights;
/* floats of the packed blob for this shape (0 = bad argument); engine as FtnPlan.engine */
size_t ftn_inception_pack_floats(int d_model, int d_ff, int n_kernels, const int* kh, const int* kw,
                                 double bottleneck_ratio, int engine);
/* Folds proj into every branch (fp64), pads channels to 16, lays the matrices out as MFMA fragments and, for the
 * split engines, splits them into pieces; writes the blob (host memory, to be copied to the device 16-byte
 * aligned) and fills *plan_out.  block0 = inception[0] (d_model -> d_ff), block2 = inception[2] (d_ff -> d_model),
 * act 0 = GELU, 1 = ReLU.  flow-timesnet_amd/pack.py is a thin wrapper of this call. */
int ftn_inception_pack_weights(const FtnInceptionBlockWeights* block0, const FtnInceptionBlockWeights* block2,
                               int d_model, int d_ff, int n_kernels, const int* kh, const int* kw,
                               double bottleneck_ratio, int act, int engine, float* blob_host, size_t blob_floats,
                               FtnPlan* plan_out);

/* ---- multi-GPU exchange of the [F] partial batch sums ------------------------------
 * A batch-sharded TimesBlock needs one exchange per call: every rank's fp64 column sums of its channel-median
 * spectrum, summed in rank order on every rank, so that all ranks select the same periods (:112 is a mean over the
 * whole batch).  Instead of a collective launch each rank's k_colsum STORES its sums straight into a slot of every
 * peer's exchange buffer - device memory of the peer, mapped here once with hipIpcOpenMemHandle, one hop over xGMI -
 * followed by a sequence word; the finalize workgroup of ftn_period_finalize[_stage_a] waits (bounded) for the
 * sequence words of all ranks in its OWN buffer and sums the slots in rank order.  No host work per call beyond
 * passing this struct; no collective; deterministic.
 *   slots[r]  rank r's exchange buffer as mapped into THIS process (slots[rank] = this rank's own hipMalloc'ed
 *             buffer of ftn_exchange_bytes(world, F_cap) bytes, zeroed once before the first call)
 *   seq       mode 0: this call's sequence number: identical on every rank, starts at 1, +1 per exchange (the two
 *             halves of the buffer alternate by seq & 1).  Ignored in mode 1.
 *   mode      (ABI 12) 0 = seq is a launch argument, set by the host before every call: the launches cannot be
 *             captured in a HIP graph (a replay would reuse the captured seq and read the peers' words of an earlier
 *             call: a silent race).  1 = capturable: seq = counter + 1, where counter is a 64-bit call counter in this rank's own
 *             buffer (byte offset ftn_exchange_counter_offset, in the line of the error word; zeroed by
 *             ftn_exchange_alloc).  k_colsum and the finalize workgroup read it, the finalize workgroup stores
 *             counter = seq once the slots are summed (or its wait timed out); nothing else writes it.  A zeroed
 *             struct is mode 0.  Other values are refused.
 * Two halves suffice, in either mode: a rank's k_colsum of call n+1 runs after its own finalize of call n, which waited
 * for every peer's k_colsum of call n, which each peer ran after its finalize of call n-1 - so a rank is at most one
 * call ahead of any peer, and what it stores into half (n+1) & 1 is no longer read.  In mode 1 the same stream order
 * gives each call on a rank one counter value: every rank that made the same calls uses the same seq, whether a call
 * was enqueued eagerly or replayed from a graph.
 * A rank that does not hear from a peer within ~2 s writes an empty descriptor (the block becomes the identity) and
 * sets the buffer's error word (ftn_exchange_error). */
#define FTN_XCHG_MAXWORLD 16
typedef struct FtnExchange {
  void* slots[FTN_XCHG_MAXWORLD];
  int32_t world, rank, F_cap;
  uint64_t seq;
  int32_t mode;
} FtnExchange;
size_t ftn_exchange_bytes(int world, int F_cap);
/* this rank's buffer on the current device (hipMalloc + zero) and its 64-byte hipIpcMemHandle_t, to be sent to the
 * other ranks by whatever channel the host has; the other ranks' handles are opened with ftn_exchange_open */
int ftn_exchange_alloc(int world, int F_cap, void** buf_out, void* handle64_out);
int ftn_exchange_open(const void* handle64, void** mapped_out);
int ftn_exchange_close(void* mapped);
int ftn_exchange_free(void* buf);
/* host-side read of the error word of this rank's own buffer (synchronises the stream): 0 = ok, 1 = a peer timed out */
int ftn_exchange_error(const FtnExchange* xch, void* stream);
/* byte offset of the mode-1 call counter (uint64) in a rank's buffer: 8 bytes past the error word, in its 256-byte line */
size_t ftn_exchange_counter_offset(int world, int F_cap);
/* host-side read of the mode-1 call counter of this rank's own buffer (synchronises the stream); -1 on a bad argument */
int64_t ftn_exchange_calls(const FtnExchange* xch, void* stream);

/* ---- multi-GPU row exchange of a series-sharded forward (ABI 13) ---------------------------------------------
 * A series-sharded TimesNet (dist.SeriesShardedTimesNet) moves fp32 rows between ranks twice per forward: the
 * partial value embeddings [B, L, D] are reduce-scattered along B (rank q receives rows q*B/W .. (q+1)*B/W - 1 of
 * every rank's partial and sums them in rank order), and the hidden rows [B/W, H, D] are all-gathered along B.  Both
 * are peer stores into IPC-mapped buffers, driven by a device call counter as FtnExchange mode 1 (there is no mode 0).
 *   slots[r]       rank r's row buffer as mapped into THIS process (slots[rank] = this rank's own buffer)
 *   rows_per_rank  R: rows each rank receives from each source (B/W)
 *   width          floats per row (L*D or H*D), a multiple of 4
 *   kind           0 = reduce-scatter: ftn_rowx_push sends source rows q*R .. q*R+R-1 to rank q (src is [W*R][width]),
 *                  ftn_rowx_reduce consumes; 1 = all-gather: ftn_rowx_push sends the same R rows to every rank (src
 *                  is [R][width]), ftn_rowx_gather consumes.  Other values are refused.
 * Buffer of one rank (ftn_rowx_bytes): two halves, each [W][R*width] floats (slot s = the rows rank s sent here) and,
 * 256-byte aligned behind them, [W][nblk] 64-bit sequence words (nblk = ceil(R*width / FTN_ROWX_CHUNK)); then one
 * 256-byte line: error word (int32 at +0), call counter (uint64 at +8), workgroup ticket (uint32 at +16).
 * Protocol, per call: seq = counter + 1, read on the device; half = seq & 1.  Every push workgroup copies one chunk of
 * FTN_ROWX_CHUNK floats into slot `rank` of one destination, releases at system scope and stores seq into the
 * destination's word [rank][chunk].  The consumer waits (bounded) for the words its chunks need, reads the slots, and
 * its last workgroup stores counter = seq.  A consumer that does not see a word within ~2 s sets the error word and
 * writes NaN rows (the heads' finite check then raises), so a lost peer never becomes plausible numbers.
 * Two halves suffice: on every rank the consumer of call n-1 runs before the push of call n (stream order).  A rank's
 * push of call n+1 into half (n+1) & 1 = (n-1) & 1 of rank q therefore follows its own consumer of call n, which
 * waited for rank q's push of call n, which rank q enqueued after its consumer of call n-1 - the last reader of that
 * half.  Every rank that made the same calls, eagerly or replayed from a graph, uses the same seq. */
#define FTN_ROWX_CHUNK 16384
typedef struct FtnRowExchange {
  void* slots[FTN_XCHG_MAXWORLD];
  int32_t world, rank;
  int32_t rows_per_rank, width;
  int32_t kind;
  int32_t reserved;
} FtnRowExchange;
/* bytes of one rank's row buffer; 0 on a bad argument (world 1..16, rows_per_rank >= 1, width >= 4 and % 4 == 0,
 * rows_per_rank * width <= 2^28) */
size_t ftn_rowx_bytes(int world, int rows_per_rank, int width);
/* this rank's buffer on the current device: uncached device memory, zeroed; an error (not plain hipMalloc) when the
 * runtime cannot allocate it.  handle64_out: its 64-byte hipIpcMemHandle_t for the other ranks' ftn_rowx_open. */
int ftn_rowx_alloc(int world, int rows_per_rank, int width, void** buf_out, void* handle64_out);
int ftn_rowx_open(const void* handle64, void** mapped_out);
int ftn_rowx_close(void* mapped);
int ftn_rowx_free(void* buf);
/* host-side reads (synchronise the stream): the error word (0 = ok, 1 = a peer timed out) and the call counter */
int ftn_rowx_error(const FtnRowExchange* xch, void* stream);
int64_t ftn_rowx_calls(const FtnRowExchange* xch, void* stream);
/* push this rank's rows (src_dev fp32, 16-byte aligned; [W*R][width] for kind 0, [R][width] for kind 1) */
int ftn_rowx_push(const float* src_dev, const FtnRowExchange* xch, void* stream);
/* kind 0 consumer: out[R][L][D] = sum over ranks s = 0..W-1 (in that order) of slot s, + add (optional: [L][D] with
 * add_bstride 0 or [R][L][D] with add_bstride L*D), then LayerNorm over D when ln_gamma / ln_beta are given.
 * width must be L*D; D a multiple of 4, <= 128; out / add / gamma / beta 16-byte aligned. */
int ftn_rowx_reduce(const FtnRowExchange* xch, int L, int D, const float* add_dev_or_null, long long add_bstride,
                    const float* ln_gamma_dev_or_null, const float* ln_beta_dev_or_null, float ln_eps, float* out_dev,
                    void* stream);
/* kind 1 consumer: out[W*R][width], row block s = the rows rank s pushed (16-byte aligned) */
int ftn_rowx_gather(const FtnRowExchange* xch, float* out_dev, void* stream);

/* ---- period selector: FFTPeriodSelector.forward (:64-159) ------------------- */
/* bytes of the DFT twiddle table for window length L */
size_t ftn_dft_table_bytes(int L);
/* fill the table (cos/sin of 2*pi*f*t/L evaluated in fp64 on the device) */
int ftn_dft_table_init(void* table_dev, int L, void* stream);
/* S1+S2 (:108-112): med[b][f] = lower-median_c |rfft_t x[b,:,c]|_f, f < L/2+1,
 * psum[f] = sum_b med[b][f] (fp64, fixed order).  med: [B][F] dev, psum: [F] dev.
 * Three kernels: one workgroup per (row, 32-bin block), or - when a row's folded samples and amplitude tile fit
 * LDS (C <= 64, e.g. L = 336) and B >= 64 - one workgroup per row with x[b] resident in LDS (bit-identical to the
 * first), folded a second time where L % 4 == 0 (agrees to 2e-6; ftn_period_spectrum_form names the choice).
 * FTN_SEL_ROW in the environment pins a form where it fits: 0 the first, 1 the row-resident, 2 the twice-folded. */
/* xch (ABI 9; may be NULL): also publish psum to slot `rank` of every rank's exchange buffer (see FtnExchange). */
/* scratch_dev (ABI 10; may be NULL): ftn_period_spectrum_scratch_bytes(B, L, C) bytes of device memory.  With it,
 * 64 < C <= 128 (d_model 128) runs the quarter-folded DFT as (row, 32-channel tile) workgroups that park their
 * amplitudes [B][F][C] there, and a second launch takes the channel medians; without it (or when the function
 * returns 0) those shapes run the (row, 32-bin block) kernel.  The rows of that form ride on gridDim.y: a batch
 * beyond 65535 rows is launched in slices of at most 65535, every row with the bits a single launch gives it. */
size_t ftn_period_spectrum_scratch_bytes(int B, int L, int C);
int ftn_period_spectrum(const float* x_dev, int B, int L, int C, const void* table_dev,
                        float* med_dev, double* psum_dev, void* stream, const FtnExchange* xch, void* scratch_dev);
/* S3-S5 (:119-157, PeriodGrouper.group :513-557, softmax/scatter :992-1009).
 * psum: [nparts][F] partial batch sums (summed in index order; nparts>1 is the
 * multi-GPU exchange of SURVEY §8e), Btotal = global batch.  Writes the
 * descriptor, amps[B][FTN_KMAX] and group weights w[B][FTN_KMAX] (both 16-byte aligned).
 * act_dtype: dtype of the caller's activations - 0 fp32, 1 bf16, 2 fp16.  For half inputs the reference
 * rounds the batch-mean spectrum and the scores (:124, :130), the returned amplitudes (:159), the softmax
 * weights (:1000) and their scatter-added group sums (:1009) to that dtype; the kernel applies the same
 * roundings (the values are still delivered as fp32).
 * max_unique / log_base: the reference's TIMES_PERIOD_MAX_UNIQ / TIMES_PERIOD_BINNING grouping variants
 * (:350-437) with the per-depth schedule already resolved by the caller; 0 / 0.0 = unset (plain
 * duplicate-merge grouping).  log_base is a double (ABI 9): the bucket is floor(log(p) / log(base) + 1e-6) with the
 * fp32 log of the period divided by (float)log(base), base in double - torch's operand order (:352).
 * Any B >= 1.  The one workgroup that selects also writes amps / w, 256 rows at a time; from a measured number of rows
 * on (FTN_FIN_ROWS=<n> in the environment forces it, 0 = never; read once per process) it leaves them to a second
 * launch, k_row_weights, one thread per row, which runs the same per-row function on the finished descriptor: same
 * bits.  ftn_period_finalize_stage_a does the same. */
int ftn_period_finalize(const double* psum_dev, int nparts, int Btotal, const float* med_dev,
                        int B, int L, int k_periods, int pmax, int min_period_threshold, int act_dtype,
                        int max_unique, double log_base, FtnDesc* desc_dev, float* amps_dev, float* weights_dev,
                        void* stream, const FtnExchange* xch);
/* (xch != NULL: psum_dev / nparts are ignored - the partial sums are the world slots of this rank's exchange buffer
 *  for this call's sequence number - xch->seq, or in mode 1 the device counter + 1 - which the kernel waits for) */
/* Host-only: PeriodGrouper.group (:513-557, env flags unset) + conv tiling for
 * periods that come from somewhere else (stub selectors in the reference tests).
 * `periods` is a host array; `desc_host` is filled on the host. */
int ftn_desc_from_periods(const int64_t* periods, int K, int L, int min_period, int max_period,
                          FtnDesc* desc_host);

/* Host-only: upper bounds for descriptors that ftn_period_finalize can write for this selector
 * configuration: returns the bound on total_px (grid pixels per batch row, > 0; < 0 on a bad argument)
 * and stores the bound on n_groups.  The selector only emits periods clamp(ceil(L/i), lo, hi) for rFFT
 * bins i (:144-145), whose pads are tiny except for bin 1, so this is far below the generic worst case. */
int ftn_selector_px_bound(int L, int k_periods, int pmax, int min_period_threshold, int* max_groups_out);

/* ---- TimesBlock conv path: _period_conv_bucketed_slicing (:955-1101) --------- */
/* Workspace / grids are sized from bounds on the device-side descriptor: max_groups >= desc->n_groups and
 * px_bound >= desc->total_px (ftn_selector_px_bound, or the exact total_px of a host-built descriptor;
 * 0 = the worst case over any max_groups distinct periods, almost 2*L*max_groups).  A descriptor that
 * exceeds them makes the call the identity y = x; nothing is ever written past the workspace.  The
 * workspace belongs to ONE call in flight: calls that may overlap (different streams, or a captured
 * graph beside eager calls) need their own.  Returns 0 for a shape it cannot run.
 * The result of a block call does not depend on the bytes the workspace held before it, for any bit pattern (NaN
 * and Inf encodings of fp32, bf16 and fp16 included); the call writes nothing outside
 * [ws_dev, ws_dev + ftn_timesblock_workspace_bytes(...)).  Nothing clears a workspace: every region is written
 * before it is read, and readers select 0 for what they mask (tests/test_gpu_workspace_hygiene.py). */
size_t ftn_timesblock_workspace_bytes(const FtnPlan* plan, int B, int L, int max_groups, int px_bound);
/* y = x + sum_g w[b,g] * (inception(fold_g(x)) - fold_g(x))[:L]  (:1041-1092, :818).
 * desc/weights are device pointers.  act_dtype (0 fp32, 1 bf16, 2 fp16) = dtype of the caller's activations:
 * x_dev / y_dev are always fp32 buffers (the caller up-casts, as the reference does for its convs, :1047-1052),
 * and for a half dtype every per-group delta, each weighted term, their sum and x + sum are rounded to it
 * exactly where the reference rounds them (:1068-1069, :1092, :818), so y holds values of that dtype.
 * flags: FTN_FWD_STAGE_A_DONE = ftn_period_finalize_stage_a already ran stage A into this workspace. */
#define FTN_FWD_STAGE_A_DONE 1
/* range_flag (ABI 9; may be NULL): one int32 the kernels can write, in device memory or in pinned host memory the
 * device can reach.  Engine f16x2 carries activations as fp16 pieces (|value| < 65504); the reference computes in
 * fp32 (:1047-1056).  Wherever a value is split - x, the stage outputs a, m, a' - and at the final y (NaN / inf) the
 * kernels test it and store 1 to *range_flag when it does not fit; the caller zeroes the word, and on 1 repeats the
 * call with a plan of engine bf16x3 (full fp32 exponent range).  Other engines never touch it. */
int ftn_timesblock_forward(const float* x_dev, float* y_dev, int B, int L, const FtnPlan* plan,
                           const float* wblob_dev, const FtnDesc* desc_dev, const float* weights_dev,
                           int max_groups, int px_bound, int act_dtype, int flags, void* ws_dev, size_t ws_bytes,
                           void* stream, int* range_flag);
/* ftn_period_finalize and stage A of the block (a = W_in1 x + b per window position, which does not depend on the
 * selector) in ONE launch: workgroup 0 is the finalize kernel and then publishes the sanitised descriptor copy at
 * the head of the workspace, the other workgroups compute stage A - the selector's single-workgroup tail (~17 us)
 * no longer leaves the chip idle.  Same plan / workspace / bounds as the ftn_timesblock_forward call that
 * follows with FTN_FWD_STAGE_A_DONE.  Bottleneck-mode plans only (mode 0).
 * The two halves can also be launched apart, on the same workspace - a batch-sharded run puts stage A between
 * issuing the exchange of the partial sums and waiting for it:  psum_dev == NULL runs stage A only (med / desc /
 * amps / weights unused),  x_dev == NULL runs S3-S5 and the descriptor copy only.  B <= 65535 whenever stage A runs
 * (its workspace holds all B rows; a call in row passes uses ftn_period_finalize). */
int ftn_period_finalize_stage_a(const double* psum_dev, int nparts, int Btotal, const float* med_dev, int B, int L,
                                int k_periods, int pmax, int min_period_threshold, int act_dtype, int max_unique,
                                double log_base, FtnDesc* desc_dev, float* amps_dev, float* weights_dev,
                                const float* x_dev, const FtnPlan* plan, const float* wblob_dev, int max_groups,
                                int px_bound, void* ws_dev, size_t ws_bytes, void* stream, int* range_flag,
                                const FtnExchange* xch);
/* The same call followed by the caller's per-block epilogue of TimesNet.forward (:2050-2058, eval mode):
 *   y = LayerNorm_C( x + (block(x) - x) ; gamma, beta, eps )
 * fused into the last kernel when d_model <= 64 (bottleneck mode), one extra in-place row pass otherwise. */
int ftn_timesblock_forward_norm(const float* x_dev, float* y_dev, int B, int L, const FtnPlan* plan,
                                const float* wblob_dev, const FtnDesc* desc_dev, const float* weights_dev,
                                int max_groups, int px_bound, int flags, const float* ln_gamma_dev,
                                const float* ln_beta_dev, float ln_eps, void* ws_dev, size_t ws_bytes, void* stream,
                                int* range_flag);
/* ---- row passes: any batch size through a bounded workspace -------------------------------------------------
 * The two calls above for any B >= 1: stages A-F are enqueued for rows [r0, r0 + n), n = min(B, rows_per_pass), pass
 * after pass on the one stream; x, y and weights advance by whole rows, the descriptor and the workspace are the same
 * for every pass.  rows_per_pass is in [1, 65535]; n * pixels per row < 2^31 as for a one-shot call; and
 *   ws_bytes >= ftn_timesblock_workspace_bytes(plan, min(B, rows_per_pass), L, max_groups, px_bound).
 * Same bits as one pass: once the selection (descriptor + weights) is fixed a row's result depends on that row of x
 * and of the weights only, and no stage reads workspace bytes the same pass has not written (see
 * ftn_timesblock_workspace_bytes), so what an earlier, possibly larger pass left behind is never seen.
 * FTN_FWD_STAGE_A_DONE is legal only when there is a single pass (ftn_period_finalize_stage_a fills a workspace of all
 * B rows).  range_flag is shared by the passes: every writer stores 1, so the word is the OR over the passes.  No
 * allocation and no synchronisation: a captured graph holds the unrolled passes.  With B <= rows_per_pass the launches
 * are exactly those of ftn_timesblock_forward / _norm.  Every argument is checked before the first launch.
 * Additions only: FTN_ABI_VERSION stays 14. */
int ftn_timesblock_forward_rows(const float* x_dev, float* y_dev, int B, int L, const FtnPlan* plan,
                                const float* wblob_dev, const FtnDesc* desc_dev, const float* weights_dev,
                                int max_groups, int px_bound, int act_dtype, int flags, void* ws_dev, size_t ws_bytes,
                                void* stream, int* range_flag, int rows_per_pass);
int ftn_timesblock_forward_norm_rows(const float* x_dev, float* y_dev, int B, int L, const FtnPlan* plan,
                                     const float* wblob_dev, const FtnDesc* desc_dev, const float* weights_dev,
                                     int max_groups, int px_bound, int flags, const float* ln_gamma_dev,
                                     const float* ln_beta_dev, float ln_eps, void* ws_dev, size_t ws_bytes,
                                     void* stream, int* range_flag, int rows_per_pass);
/* Host-only: the largest legal rows_per_pass (<= 65535, rows * pixels per row < 2^31) whose workspace is at most
 * ws_cap_bytes; ws_cap_bytes = 0 means no cap.  0 when a single row does not fit (or the shape is bad). */
int ftn_timesblock_rows_per_pass(const FtnPlan* plan, int L, int max_groups, int px_bound, size_t ws_cap_bytes);
/* out[row][:] = LayerNorm_C( x[row][:] + (new[row][:] - x[row][:]) ) for rows x C fp32 matrices (in place
 * allowed: out == new).  Used when a block returns x unchanged (no valid period, :796-797). */
int ftn_residual_layernorm(const float* x_dev, const float* new_dev, float* out_dev, long long rows, int C,
                           const float* ln_gamma_dev, const float* ln_beta_dev, float ln_eps, void* stream);

/* ---- kernel forms (ABI 11, host-only) -------------------------------------------- */
/* Which kernel form each stage of ftn_timesblock_forward takes for a plan, shape, activation dtype and input
 * alignment.  ftn_timesblock_forward makes its choice through the same host function, so the report is what runs;
 * the environment switches the library reads (FTN_MLP_POS, FTN_OUT_H, FTN_MLP_U1, FTN_R_KEEPS_X,
 * FTN_CONV_GENERIC) are reflected.  y is taken to be 16-byte aligned (callers allocate it). */
#define FTN_FORM_CONV_FP32 0          /* k_conv (exact fp32 MFMA)                                        */
#define FTN_FORM_CONV_BF 1            /* k_conv_bf<conv_n, nsplit>                                        */
#define FTN_FORM_CONV_BF_FAST 2       /* k_conv_bf_fast<nsplit, conv_n>                                   */
#define FTN_FORM_C_MLP 0              /* k_mlp (fp32)                                                     */
#define FTN_FORM_C_GENERIC 1          /* the chain as generic pointwise launches (k_pw / k_ew_ident)      */
#define FTN_FORM_C_MLP_BF 2           /* k_mlp_bf<nsplit>                                                 */
#define FTN_FORM_C_MLP_BF_U1 3        /* k_mlp_bf_u1<nsplit> (one 16-pixel unit per wave)                 */
#define FTN_FORM_C_MLP_BF_C128 4      /* k_mlp_bf_c128<nsplit> (d_model 128, three kernels, mid 32)       */
#define FTN_FORM_C_MLP_POS64 5        /* k_mlp_pos, d_model-64 shape (position-major, R group-summed)     */
#define FTN_FORM_C_MLP_POS128 6       /* k_mlp_pos, d_model-128 shape                                     */
#define FTN_FORM_E_OUT 0              /* k_out, general form                                              */
#define FTN_FORM_E_OUT_FAST 1         /* k_out, FAST form (16 pixels per wave)                            */
#define FTN_FORM_E_OUT_H 2            /* k_out_h (stage E on the 16-bit pipe)                             */
#define FTN_FORM_E_OUT_MERGED 3       /* k_out of a merged-conv (mode 1) plan                             */
typedef struct FtnForms {
  int32_t mode;        /* plan mode: 0 bottleneck branches, 1 one merged conv                               */
  int32_t act;         /* ACT template argument: 0 GELU, 1 ReLU                                             */
  int32_t nsplit;      /* activation pieces of the split conv engine: 3 bf16x3, 2 f16x2, 1 bf16; 0 fp32      */
  int32_t xvec;        /* x is read with 16-byte vector loads (C % 4 == 0 and x 16-byte aligned)            */
  int32_t yvec;        /* y is written with 16-byte vector stores                                           */
  int32_t stage_a_epi; /* epilogue of stage A (k_pw / k_finalize_pw): 0 fp32, 2 bf16 pieces, 3 f16x2 pieces;
                          -1 for mode 1 (k_embed)                                                           */
  int32_t conv;        /* FTN_FORM_CONV_*                                                                   */
  int32_t conv_n;      /* k_conv_bf: output tiles per workgroup (NCO); k_conv_bf_fast: input groups (NCI)   */
  int32_t stage_c;     /* FTN_FORM_C_*                                                                      */
  int32_t r_keeps_x;   /* stage C leaves x inside R (stage E does not add it again)                         */
  int32_t r_summed;    /* R is already summed over the groups with their weights                            */
  int32_t stage_e;     /* FTN_FORM_E_*                                                                      */
  int32_t half_round;  /* act_dtype != 0: stage E rounds every per-group term to the half dtype             */
  int32_t reserved[3];
} FtnForms;
/* x_misalign: byte offset of x from a 16-byte boundary (0 = aligned).  Returns 0, or < 0 on a bad argument. */
int ftn_timesblock_forms(const FtnPlan* plan, int B, int L, int act_dtype, int x_misalign, FtnForms* forms_out);
/* The form ftn_period_spectrum takes (scratch: whether the caller passes the scratch buffer):
 * 0 k_spectrum, 1 k_spectrum_row, 2 k_spectrum_rowq, 3 channel-tiled k_spectrum_rowq + k_median_rows;
 * plus 4 when x is read with 16-byte vector loads.  < 0 on a bad argument. */
int ftn_period_spectrum_form(int B, int L, int C, int x_misalign, int scratch);

/* ---- LowRankTemporalContext (:1340-1371) -------------------------------------- */
/* basis buffer: (L+1)*R floats = basis[l][r] (DCT-II columns r=1..R, centred over l,
 * unit L2 norm, :1344-1351) followed by the R residual column means */
size_t ftn_lrtc_basis_floats(int L, int R);
int ftn_lrtc_basis(float* basis_dev, int L, int R, void* stream);
/* out[b][l][n] = (x ? x[b][l][n] : 0) + scale * sum_r basis_c[l][r] coeff[b][n][r]
 * with the time-mean removed (:1368-1371).  scale_dev: 1 float on the device. */
int ftn_lrtc_forward(const float* coeff_dev, const float* basis_dev, const float* scale_dev,
                     const float* x_dev_or_null, float* out_dev, int B, int L, int N, int R,
                     void* stream);
/* The form ftn_lrtc_forward takes (host-only; the launch dispatches through the same function):
 *   bit 0      FTN_LRTC_VEC   16-byte stores of out (and loads of x): N % 4 == 0, out and x 16-byte aligned
 *   bit 1      FTN_LRTC_ADDX  fused x +
 *   bit 2      FTN_LRTC_WIDE  a lane's 4 R coefficients come in as 16-byte loads: R == RT, N >= 4 and coeff 16-byte
 *                             aligned (a lane whose quad crosses N, and every lane otherwise, loads them one by one)
 *   bits 4-9   RT: the rank padded to 4 | 8 | 16 | 32
 *   bits 12-15 nqb / 64: lanes spanning one workgroup's series quads (64 | 128 | 256); gridDim.x = ceil(N / (4 nqb))
 * misalign_or: ((out | x) & 15) | (coeff & 15) << 4, the pointers as byte addresses (x left out when addx == 0).
 * Returns < 0 on a bad argument. */
#define FTN_LRTC_VEC 1
#define FTN_LRTC_ADDX 2
#define FTN_LRTC_WIDE 4
int ftn_lrtc_form(int N, int R, int addx, int misalign_or);

/* ---- model shell around the block stack (TimesNet.forward) ------------------------
 * Every entry point of the shell - narrow (D <= 128, declared first), wide (ftn_*_wide_*, 128 < D <= 512) and _rms -
 * is defined in csrc/shell_api.hip: one body per operation checks the arguments, and the kernels are in
 * csrc/shell.hip (narrow), csrc/shell_wide.hip (wide) and csrc/timeproj.hip.  The entry names its width; D outside
 * that width's range is a bad argument, never a switch to the other width.  A bad argument returns < 0 before any
 * launch, with a message that starts with the entry's name.  The rules, once per operation (strides in elements):
 *   every operation   required pointers non-null; every count >= 1; D a multiple of 4 within the width's range
 *   heads             rows % S == 0; 1 <= hist <= S; hidden, w_mu, w_sigma 16-byte aligned
 *                     wide only: every other operand 4-byte aligned
 *   embedding         gamma and beta both or neither (_rms: both); out, add, gamma, beta 16-byte aligned;
 *                     add_bstride % 4 == 0.  wide only: B * L <= 0x7fffffff; x and W 4-byte aligned
 *   embedding rows    out 16-byte aligned; out_bstride % 4 == 0, and >= L * D when B > 1
 *                     wide only: B * L <= 0x7fffffff; x and W 4-byte aligned
 *   ring              0 <= head < L; gamma / beta as the embedding; V, out, add, gamma, beta 16-byte aligned;
 *                     add_bstride % 4 == 0 and >= 0.  wide only: B * L <= 0x7fffffff
 *   time projection   seq, hidden 16-byte aligned; W_t, b_t 4-byte aligned; B * ceil(D / 64) <= 0x7fffffff and
 *                     ceil(S / 16) <= 65535.  No difference between the widths.
 *   form queries      N (L, S) >= 1; D as above; every misalign one of 0, 4, 8, 12
 * The "wide only" checks are a deliberate difference: the narrow entry points accept what they always accepted. */
/* Rate / dispersion heads (:2066-2102), one pass over hidden[rows = B*S][D] (the output of
 * forecast_time_proj, time-major):
 *   pre        = hidden W_mu^T + b_mu + tail[b, min(s, hist-1), :] (+ late[b, s, :])
 *   rate       = softplus(pre) + 1e-6
 *   dispersion = softplus(hidden W_sigma^T + b_sigma) + floor + 1e-6
 * W_* are nn.Linear weights [N][D]; tail points at x[b=0, T-hist, 0] with batch stride tail_bstride
 * (elements); late (optional) is gate * late_bias laid out [.., S, N] with batch stride late_bstride
 * (0 = shared by the batch); floor is min_sigma_vector[N] or the scalar.  *bad_flag_dev gets bit 0 / 1
 * OR-ed in when a rate / dispersion is not finite and > 0 (the reference raises RuntimeError, :2095-2098);
 * the caller zeroes it. */
int ftn_head_forward(const float* hidden_dev, long long rows, int S, int D, int N, const float* w_mu_dev,
                     const float* b_mu_dev, const float* w_sigma_dev, const float* b_sigma_dev,
                     const float* tail_dev, long long tail_bstride, int hist, const float* late_dev_or_null,
                     long long late_bstride, const float* floor_vec_dev_or_null, float floor_scalar,
                     float* rate_dev, float* disp_dev, int* bad_flag_dev, void* stream);

/* Value embedding of DataEmbedding.forward (:1283-1325) with everything row-linear folded into `add`:
 *   out[b][l][:] = x[b][l][:] W^T + add[b?][l][:]      (+ LayerNorm over D when gamma/beta are given)
 * x: the [B, L, N] input window (rows contiguous, batch stride x_bstride elements); W: nn.Linear weight
 * [D][N]; add: optional [L][D] (add_bstride 0) or [B][L][D] holding bias + positional/time-feature term
 * (+ the low-rank temporal context and constant context bias pushed through W, :1958-1996, so the
 * [B, L, N] context tensor is never written). */
int ftn_embed_forward(const float* x_dev, long long x_bstride, int B, int L, int N, const float* w_dev, int D,
                      const float* add_dev_or_null, long long add_bstride, const float* ln_gamma_dev_or_null,
                      const float* ln_beta_dev_or_null, float ln_eps, float* out_dev, void* stream);

/* The GEMM of ftn_embed_forward alone (no add, no LayerNorm), row (b, l) of x W^T stored at
 * out + b * out_bstride + l * D: same kernels, form selection and K order, so each row is bit-identical to
 * the one ftn_embed_forward computes before its epilogue.  The recursive forecaster appends a step's B new
 * rows (L = 1) to its ring of embedded rows with it. */
int ftn_embed_rows_strided(const float* x_dev, long long x_bstride, int B, int L, int N, const float* w_dev, int D,
                           float* out_dev, long long out_bstride, void* stream);

/* Embedding of a sliding window from a ring of stored x W^T rows V [B][L][D] whose oldest row is slot `head`:
 *   out[b][t][:] = V[b][(head + t) mod L][:] + add[b?][t][:]      (+ LayerNorm over D when gamma/beta are given)
 * with ftn_embed_forward's epilogue arithmetic (bit-identical to it on the equivalent window).  add optional
 * ([L][D] with add_bstride 0, or [B][L][D]). */
int ftn_embed_ring(const float* v_dev, int B, int L, int D, int head, const float* add_dev_or_null,
                   long long add_bstride, const float* ln_gamma_dev_or_null, const float* ln_beta_dev_or_null,
                   float ln_eps, float* out_dev, void* stream);

/* ---- kernel forms of the model shell (ABI 14, host-only) ------------------------------------------------------
 * Which kernel the embedding entry points (ftn_embed_forward, ftn_embed_rows_strided) and ftn_head_forward run.
 * The launches dispatch through the same host functions, so the report is what runs; the environment switches the
 * library reads (FTN_EMBED_F32, FTN_EMBED_RT, FTN_HEAD_F32) are reflected.  Encoding (both functions):
 *   bit 0      FTN_SHELL_BF   1 = bf16x3 on the 16-bit matrix pipe (k_embed_in_bf / k_head_bf), 0 = exact fp32 MFMA
 *   bit 1      FTN_SHELL_VEC  16-byte vector loads / stores (always set with FTN_SHELL_BF)
 *   bits 4-7   first template argument:  NO (embedding: 4 | 8), NT (k_head_bf: 4 | 2), NS (k_head: 1 | 2 | 4 | 8)
 *   bits 8-11  second template argument: RT (embedding: 16-row tiles per wave), NS32 (k_head_bf), 0 for k_head
 *   bits 16-27 heads only: the cap on gridDim.y; a workgroup walks more than one 64-row group of `hidden` when
 *              rows > 64 * cap
 * *_misalign: byte offset of the pointer from a 16-byte boundary (0, 4, 8 or 12); for the heads the OR of the
 * offsets of tail, late, rate and disp (hidden and the weights must be aligned).  Strides in elements, as the entry
 * points take them.  Returns < 0 on a bad argument. */
#define FTN_SHELL_BF 1
#define FTN_SHELL_VEC 2
int ftn_embed_form(int N, int D, long long x_bstride, int x_misalign, int w_misalign);
int ftn_head_form(int N, int D, long long tail_bstride, long long late_bstride, int misalign_or);

/* Time projection between the block stack and the heads (forecast_time_proj, :2063-2066):
 *   hidden[b][s][:] = b_t[s] + sum_l W_t[s][l] seq[b][l][:]
 * seq [B][L][D] and hidden [B][S][D] contiguous fp32, 16-byte aligned; W_t [S][L] with row stride L and b_t [S]
 * need only 4-byte alignment (they may be the row slice weight[-S:]).  Any B, L, S >= 1.
 * The order in which the L terms of an output element are added depends on (L, S, D) alone: row b comes out
 * bit-identical whatever B is and whichever rows share the call.  One launch, no workspace.
 * ftn_timeproj_form (host-only; the launch dispatches through the same function): 0 = k_timeproj_row (S == 1, fp32
 * FMA on the VALU); otherwise FTN_SHELL_BF (bf16x3 on the 16-bit matrix pipe, k_timeproj_bf<NST, WV>) with
 *   bit 1      FTN_SHELL_VEC  WV: W_t is read with 16-byte loads (L % 4 == 0 and wt_misalign == 0)
 *   bits 4-7   NST: 16-step tiles of S a wave accumulates (1 | 2 | 4 | 6); gridDim.y = ceil(S / (16 NST))
 *   bits 8-11  waves of a workgroup, which share the K-32 slabs of L (8)
 * Returns < 0 on a bad argument. */
int ftn_timeproj_forward(const float* seq_dev, int B, int L, int D, const float* wt_dev, const float* bt_dev, int S,
                         float* hidden_dev, void* stream);
int ftn_timeproj_form(int L, int S, int D, int wt_misalign);

/* ---- model shell at 128 < d_model <= 512 (kernels: csrc/shell_wide.hip, csrc/timeproj.hip) --------------------
 * These entry points are additions only: no earlier declaration changed, so FTN_ABI_VERSION stays 14.  The entry
 * points above keep their limit (D <= 128), forms and bits; each one below takes the arguments of its narrow
 * counterpart with the same meaning and "enqueue only, no hidden allocation" convention, for D a multiple of 4 with
 * 128 < D <= 512, under the argument rules at the head of the shell section.  Products are bf16x3
 * on the 16-bit matrix pipe.  The order of the K additions of an output element and of the LayerNorm reductions is a
 * function of (N, D, form) alone: a row's bits do not depend on B, on its position in the batch or on which rows
 * share the call; no atomics on outputs, no split of K across workgroups.
 *
 * Embedding (k_embed_wide_bf<NO, RT, VEC>): a workgroup of four waves owns 16 RT rows and sees their whole output
 * row; wave w takes the 16 NO-column slab w of D.  x is read from HBM once (split once per workgroup, shared through
 * LDS), W from L2 once per workgroup.  The wide rows entry writes the GEMM alone: its rows are bit-identical to what the wide forward holds
 * before its epilogue.  The wide ring (k_embed_wide_ring) shares the epilogue function of the GEMM kernel.
 * ftn_embed_wide_form (host-only; the launch dispatches through the same function):
 *   bit 0      FTN_SHELL_BF   always set
 *   bit 1      FTN_SHELL_VEC  16-byte loads of x and W: N % 4 == 0, x_bstride % 4 == 0 and both bases aligned;
 *                             otherwise guarded 4-byte loads with the same arithmetic
 *   bits 4-7   NO: 16-column tiles of a wave's slab (4 for D <= 256, else 8)
 *   bits 8-11  RT: 16-row tiles of a workgroup (4)
 *
 * Heads: ftn_head_wide_form returns 0 for k_head_wide_f32 (operands that are not vectorisable, as FTN_SHELL_VEC of
 * ftn_head_form: plain fp32 FMAs in k order), otherwise FTN_SHELL_BF | FTN_SHELL_VEC (k_head_wide_bf<NT>) with
 *   bits 4-7   NT: 16-series tiles of a workgroup (2 for D <= 256, else 1); the split weights of both heads for
 *              ceil(D / 32) K-32 slabs sit in LDS (6 KB per tile and slab)
 *   bits 16-27 the cap on gridDim.y = ceil(256 W / ceil(N / (16 NT))) with W the workgroups whose LDS fits a CU's
 *              160 KB; a workgroup walks more than one 64-row group of `hidden` when rows > 64 * cap
 *
 * Time projection: ftn_timeproj_wide_form has the encoding of ftn_timeproj_form; S > 1 runs k_timeproj_bf as it is,
 * 0 (S == 1) is k_timeproj_row_wide (128-column slabs across gridDim.y, 16 row groups whatever D is). */
int ftn_embed_wide_forward(const float* x_dev, long long x_bstride, int B, int L, int N, const float* w_dev, int D,
                           const float* add_dev_or_null, long long add_bstride, const float* ln_gamma_dev_or_null,
                           const float* ln_beta_dev_or_null, float ln_eps, float* out_dev, void* stream);
int ftn_embed_wide_rows_strided(const float* x_dev, long long x_bstride, int B, int L, int N, const float* w_dev,
                                int D, float* out_dev, long long out_bstride, void* stream);
int ftn_embed_wide_ring(const float* v_dev, int B, int L, int D, int head, const float* add_dev_or_null,
                        long long add_bstride, const float* ln_gamma_dev_or_null, const float* ln_beta_dev_or_null,
                        float ln_eps, float* out_dev, void* stream);
int ftn_head_wide_forward(const float* hidden_dev, long long rows, int S, int D, int N, const float* w_mu_dev,
                          const float* b_mu_dev, const float* w_sigma_dev, const float* b_sigma_dev,
                          const float* tail_dev, long long tail_bstride, int hist, const float* late_dev_or_null,
                          long long late_bstride, const float* floor_vec_dev_or_null, float floor_scalar,
                          float* rate_dev, float* disp_dev, int* bad_flag_dev, void* stream);
int ftn_timeproj_wide_forward(const float* seq_dev, int B, int L, int D, const float* wt_dev, const float* bt_dev,
                              int S, float* hidden_dev, void* stream);
int ftn_embed_wide_form(int N, int D, long long x_bstride, int x_misalign, int w_misalign);
int ftn_head_wide_form(int N, int D, long long tail_bstride, long long late_bstride, int misalign_or);
int ftn_timeproj_wide_form(int L, int S, int D, int wt_misalign);

/* ---- RMS norm epilogue of the value embedding (embed_norm_mode "rms"; kernels: csrc/shell.hip, shell_wide.hip) --
 * These entry points are additions only: no earlier declaration changed, so FTN_ABI_VERSION stays 14.
 *
 * Each takes the argument list of its LayerNorm counterpart (ftn_embed_forward, ftn_embed_ring, ftn_embed_wide_forward,
 * ftn_embed_wide_ring) with the same meaning, argument rules and "enqueue only, no allocation" convention, and closes
 * a row with the reference's RMS norm instead
 * (models/timesnet.py:1153-1158), in fp32:
 *   v     = x[b][l][:] W^T + add[b?][l][:]        (ring: V[b][(head + t) mod L][:] + add[b?][t][:])
 *   ss    = sum_d v[d]^2
 *   scale = 1 / sqrt(ss / D + eps)
 *   out   = (v * scale) * gamma + beta
 * gamma and beta [D] are required here: a null one is a bad argument (< 0), reported before any launch.
 * The kernels and forms are those of the counterparts (ftn_embed_form / ftn_embed_wide_form answer for both): the
 * norm is an argument of the kernel, not another kernel.  ss is added up in the order of the LayerNorm mean - a pair
 * tree over the four columns of each of the lane's column tiles, the tiles in order, the four lanes of a row (xor 16,
 * 32), and beyond d_model 128 the four column slabs in slab order through LDS with one barrier (LayerNorm: two); a slab
 * past D adds an exact zero.  Nothing is pre-scaled against overflow: a row whose squares overflow fp32 has
 * scale = 1 / sqrt(inf) = 0 and comes out as beta, as the reference's fp32 rsqrt(inf) gives it.  The norm is compiled
 * without FMA contraction in the GEMM kernels and in the ring kernels alike, so a ring row is bit-identical to the row
 * of the one-pass call on the equivalent window on every form and at every D (LayerNorm: on some narrow forms only).
 * A row's bits do not depend on B, on its position in the batch or on which rows share the call. */
int ftn_embed_forward_rms(const float* x_dev, long long x_bstride, int B, int L, int N, const float* w_dev, int D,
                          const float* add_dev_or_null, long long add_bstride, const float* gamma_dev,
                          const float* beta_dev, float eps, float* out_dev, void* stream);
int ftn_embed_ring_rms(const float* v_dev, int B, int L, int D, int head, const float* add_dev_or_null,
                       long long add_bstride, const float* gamma_dev, const float* beta_dev, float eps,
                       float* out_dev, void* stream);
int ftn_embed_wide_forward_rms(const float* x_dev, long long x_bstride, int B, int L, int N, const float* w_dev, int D,
                               const float* add_dev_or_null, long long add_bstride, const float* gamma_dev,
                               const float* beta_dev, float eps, float* out_dev, void* stream);
int ftn_embed_wide_ring_rms(const float* v_dev, int B, int L, int D, int head, const float* add_dev_or_null,
                            long long add_bstride, const float* gamma_dev, const float* beta_dev, float eps,
                            float* out_dev, void* stream);

/* ---- scoring a forecast (losses.py:27-58, train.py:675-765 of the reference) -------------------------
 * These entry points are additions only: no earlier declaration changed, so FTN_ABI_VERSION stays 14.
 *
 * ftn_score_columns (k_score_cols<CPL>): one pass over y, rate, dispersion [B][H][N] (fp32, rows N elements apart,
 * N fastest, each with its own batch stride in elements) and an optional mask (contiguous [B][H][N]; mask_kind 0
 * none, 1 uint8, 2 fp32 where nonzero is true).  Per element, in the reference's words:
 *   yc = y < 0 ? 0 : y,  alpha = max(dispersion, eps),  mu = max(rate, eps)          (a NaN stays a NaN)
 *   ll = lgamma(yc + 1/alpha) - lgamma(1/alpha) - lgamma(yc + 1) - log1p(alpha mu) / alpha
 *        + yc (log alpha + log mu - log1p(alpha mu))
 *   valid = isfinite(yc) & isfinite(mu) & isfinite(alpha) & mask
 * ll is evaluated in fp64 (Stirling's series above 8 after an upward shift; the last addend as
 * -yc log1p(1 / (alpha mu))) and rounded once to fp32; that fp32 value goes to ll_out (optional, contiguous
 * [B][H][N], 0 where invalid) and, negated, into the column's fp64 sum.  The sMAPE term of a valid element with
 * finite |y| > 1e-8 (the unclamped y) is 2 |rate - y| / (|y| + |rate|) in fp32 operations, summed in fp64.
 * An invalid element contributes NOTHING (the reference multiplies by a 0 weight, so one masked-out NaN makes its
 * mean NaN: DESIGN.md section 8).
 * part_out[b N + n] is column (b, n)'s record.  Its sums run over h ascending; H is cut into nseg <= 8 segments of
 * seg = max(4, ceil(H / 8)) rows, one wave each, whose partial sums are added in ascending order: the order is a
 * function of H alone, no atomics, and a column's record is the same bits whatever B is and whichever rows share
 * the call.  H N and B N must fit an int32.
 * ftn_score_form (host-only; the launch dispatches through the same function):
 *   bit 1      FTN_SHELL_VEC  k_score_cols<4>: 16-byte loads, four columns per lane (N % 4 == 0, every batch stride
 *              a multiple of 4, misalign_or == 0); otherwise k_score_cols<1>, one column per lane
 *   bits 4-7   nseg, the waves of a workgroup
 *   bits 8-27  seg, the rows of a segment
 * misalign_or: the OR of (address & 15) of y, rate, dispersion, ll_out and an fp32 mask, and of (address & 3) << 2
 * of a uint8 mask. */
typedef struct FtnScorePart {
  double nll_sum;      /* sum of -ll over the valid elements                          */
  double smape_sum;    /* sum of the sMAPE terms that count                           */
  int32_t nll_cnt;     /* valid elements                                              */
  int32_t smape_cnt;   /* sMAPE terms that count                                      */
} FtnScorePart;
int ftn_score_form(int H, int N, long long y_bstride, long long rate_bstride, long long disp_bstride,
                   int misalign_or);
int ftn_score_columns(const float* y_dev, long long y_bstride, const float* rate_dev, long long rate_bstride,
                      const float* disp_dev, long long disp_bstride, const void* mask_dev, int mask_kind, float eps,
                      int B, int H, int N, FtnScorePart* part_out_dev, float* ll_out_dev, void* stream);
/* ftn_score_fold (k_score_fold): acc[slot] += part[b N + n], field by field and IN PLACE, one record at a time in
 * ascending (b, n) order for every slot, so folding batch X and then batch Y leaves the bits that folding
 * cat([X, Y]) leaves.  ids_kind:
 *   0  slot = n (ids, order, seg_start null; N <= n_slots)
 *   1  slot = ids[n], ids int64 [N], distinct within the row
 *   2  any ids, e.g. per-sample [B][N] with repeats: order int64 [B N] is the stable argsort of the ids and
 *      seg_start int64 [n_slots + 1] the first position of every slot in it; one thread owns a slot and walks
 *      its segment
 * An id outside [0, n_slots) sets bit 0 of *err_dev (int32, caller-owned, never cleared here) and its record is
 * dropped; nothing is read or written out of bounds. */
int ftn_score_fold(const FtnScorePart* part_dev, int B, int N, int ids_kind, const long long* ids_dev,
                   const long long* order_dev, const long long* seg_start_dev, FtnScorePart* acc_dev, int n_slots,
                   int* err_dev, void* stream);

/* ---- refitting the heads: the gradient of that likelihood (losses.py:27-58 under autograd; csrc/headfit.hip) ----
 * Additions only: FTN_ABI_VERSION stays 14.
 *
 * ftn_nb_nll_grad: operands, mask, clamps and validity as ftn_score_columns.  Per element it writes the derivatives
 * of the LOG-likelihood (contiguous fp32 [B][H][N]):
 *   g_rate = (yc - mu) / (mu (1 + alpha mu))
 *   g_disp = (log1p(alpha mu) - [psi(yc + 1/alpha) - psi(1/alpha)]) / alpha^2 + (yc - mu) / (alpha (1 + alpha mu))
 * evaluated in fp64 and rounded once; the digamma difference is sc_dpsi (csrc/ftn_nbmath.h, 5e-12 relative), never
 * two digammas subtracted.  g_rate is 0 where rate < eps and g_disp is 0 where dispersion < eps (the clamp is
 * active); an element that is masked out or not finite gets two exact zeros and adds nothing to the sums.
 * Two launches.  k_nb_grad<V>: a grid of nparts <= FTN_NBG_PARTS_MAX workgroups of 256 walks the elements and leaves
 * in the workspace, per workgroup, the fp64 sums of ll and of the valid count.  k_nb_grad_fold: adds them in
 * ascending order and writes
 *   loss_dev[0] = -sum ll / max(count, 1)          loss_dev[1] = -1 / max(count, 1)
 * and, with scaled = 1, multiplies g_rate and g_disp by loss_dev[1] in place: they are then the gradients of the
 * loss.  With scaled = 0 the derivatives stay raw and a later kernel applies the device word.  Nothing synchronises,
 * there are no atomics, and every sum's order is a function of the shape alone; the workspace may hold anything.
 * ftn_nb_nll_grad_workspace gives its bytes (0 for a bad shape).  H N and B N must fit an int32; g_rate and g_disp
 * are distinct buffers that overlap no operand.
 * ftn_nb_nll_grad_form (host-only; the launch dispatches through the same function):
 *   bit 1      FTN_SHELL_VEC  k_nb_grad<4>: 16-byte loads and stores, four elements per lane (H N % 4 == 0, every
 *              batch stride a multiple of 4, misalign_or == 0); otherwise k_nb_grad<1>
 *   bits 4-14  nparts
 * misalign_or: the OR of (address & 15) of y, rate, dispersion, g_rate, g_disp and an fp32 mask, and of
 * (address & 3) << 2 of a uint8 mask. */
#define FTN_NBG_PARTS_MAX 1024
int ftn_nb_nll_grad_form(int B, int H, int N, long long y_bstride, long long rate_bstride, long long disp_bstride,
                         int misalign_or);
size_t ftn_nb_nll_grad_workspace(int B, int H, int N);
int ftn_nb_nll_grad(const float* y_dev, long long y_bstride, const float* rate_dev, long long rate_bstride,
                    const float* disp_dev, long long disp_bstride, const void* mask_dev, int mask_kind, float eps,
                    int B, int H, int N, float* g_rate_dev, float* g_disp_dev, float* loss_dev, void* workspace_dev,
                    size_t workspace_bytes, int scaled, void* stream);

/* The heads for a refit (csrc/headfit.hip; additions only).  R = B S rows of hidden [R][D], D a multiple of 4 up to 512.
 *
 * ftn_head_fit_forward: ftn_head_forward / ftn_head_wide_forward (whichever takes D) with two more outputs - the same
 * kernels, form choice and rate / dispersion bits, every operand 4-byte aligned - sig_mu / sig_sigma [R][N],
 * 16-byte aligned: softplus' derivative at both pre-activations, sigmoid(t) for t <= 20 and 1 above (torch's softplus
 * backward).  One launch.
 *
 * ftn_head_backward: with G_mu = g_rate sig_mu scale and G_sg = g_disp sig_sigma scale ([R][N]; g_* the raw
 * derivatives of ftn_nb_nll_grad with scaled = 0, scale its device word loss_dev + 1; G_mu is also the late bias'
 * gradient),
 *   dW_mu[n][d] = sum_r G_mu[r][n] hidden[r][d]     db_mu[n] = sum_r G_mu[r][n]       (the same pair for sigma)
 *   d_hidden    = G_mu W_mu + G_sg W_sigma          (when d_hidden is given; it needs both weights, 16-byte aligned)
 * Rows are cut into chunks of 256 (of ceil(R / FTN_HEADFIT_CHUNKS_MAX), made even, beyond 256 chunks); a chunk's
 * partial [2][N][D + 1] (column D: the bias) goes to the caller's workspace (ftn_head_backward_workspace bytes, 0 for
 * a bad shape; whatever it held before) and a second kernel adds the chunks in ascending order: the same bits on
 * every run.  ftn_head_backward_form (host-only; the launch dispatches through the same function):
 *   bits 0-3   FTN_HEADFIT_COLSUM  N <= 4 and hidden 16-byte aligned: lanes own float4 columns of hidden and a
 *                                  workgroup's row lanes are added in ascending order
 *              FTN_HEADFIT_MFMA    otherwise: [32 n x 32 d] tiles on v_mfma_f32_32x32x2_f32, K = the chunk's rows
 *   bits 4-12  the number of chunks
 * misalign_or: (address & 15) of hidden. */
#define FTN_HEADFIT_COLSUM 1
#define FTN_HEADFIT_MFMA 2
#define FTN_HEADFIT_CHUNKS_MAX 256
int ftn_head_backward_form(long long R, int N, int D, int misalign_or);
size_t ftn_head_backward_workspace(long long R, int N, int D);
int ftn_head_fit_forward(const float* hidden_dev, long long rows, int S, int D, int N, const float* w_mu_dev,
                         const float* b_mu_dev, const float* w_sigma_dev, const float* b_sigma_dev,
                         const float* tail_dev, long long tail_bstride, int hist, const float* late_dev_or_null,
                         long long late_bstride, const float* floor_vec_dev_or_null, float floor_scalar,
                         float* rate_dev, float* disp_dev, float* sig_mu_dev, float* sig_sigma_dev, int* bad_flag_dev,
                         void* stream);
int ftn_head_backward(const float* hidden_dev, long long R, int N, int D, const float* g_rate_dev,
                      const float* g_disp_dev, const float* sig_mu_dev, const float* sig_sigma_dev,
                      const float* scale_dev, const float* w_mu_dev, const float* w_sigma_dev, float* dw_mu_dev,
                      float* db_mu_dev, float* dw_sigma_dev, float* db_sigma_dev, float* d_hidden_dev_or_null,
                      void* workspace_dev, size_t workspace_bytes, void* stream);

/* The time projection's backward, for a refit of the whole output side (csrc/timeproj_bwd.hip; additions only:
 * FTN_ABI_VERSION stays 14).  seq [B][L][D] is ftn_timeproj_forward's input, d_hidden [B][S][D] the d_hidden of
 * ftn_head_backward (the loss scale is in it); both contiguous fp32 and 16-byte aligned (an operand off that grid is
 * rejected before any launch), D a multiple of 4 from 4 to 512, B, L, S >= 1 (S == 1: the recursive model, whose
 * weight is the last row of the [pred_len][L] matrix).
 *   dW_t[s][l] = sum_b sum_d d_hidden[b][s][d] seq[b][l][d]        db_t[s] = sum_b sum_d d_hidden[b][s][d]
 * dW_t [S][L] and db_t [S] are contiguous, 4-byte aligned, written with plain stores and nothing around them is
 * touched.  Batch rows are cut into chunks of 8 (of ceil(B / FTN_TIMEPROJ_BWD_CHUNKS_MAX) beyond 256 chunks); a
 * chunk's partial [S][L + 1] (column L: the bias) goes to the caller's workspace (ftn_timeproj_backward_workspace
 * bytes, 0 for a bad shape; whatever it held before) and a second kernel adds the chunks in a fixed order (chunks
 * c, c + 16, ... ascending, then the 16 sums ascending).  No atomics and no library GEMM: every sum's order is a
 * function of (B, L, S, D) alone, the same bits on every run, and every product is an exact fp32 fmaf step
 * (v_mfma_f32_32x32x2_f32; no operand is split).  Two launches, enqueued only.
 * ftn_timeproj_backward_form (host-only; the launch dispatches through the same function):
 *   bits 0-3   FTN_TIMEPROJ_BWD_MFMA  [32 s x 32 l] tiles, K = the (b, d) pairs of the chunk's batch rows, dealt to the
 *                                     four waves of a workgroup and added in wave order
 *   bits 4-12  the number of chunks
 * misalign_or: the OR of (address & 15) of seq and d_hidden; anything but 0 is an error here as in the launch. */
#define FTN_TIMEPROJ_BWD_MFMA 1
#define FTN_TIMEPROJ_BWD_CHUNKS_MAX 256
int ftn_timeproj_backward_form(int B, int L, int S, int D, int misalign_or);
size_t ftn_timeproj_backward_workspace(int B, int L, int S, int D);
int ftn_timeproj_backward(const float* seq_dev, const float* d_hidden_dev, int B, int L, int S, int D, float* dw_t_dev,
                          float* db_t_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- cached refit: the frozen backbone's output kept per item (csrc/timeproj.hip, timeproj_bwd.hip, refit_rows.hip) --
 * These entry points are additions only: no earlier declaration changed, so FTN_ABI_VERSION stays 14.
 *
 * Row-mapped forms of the two readers of seq.  seq is an item store [n_items][L][D] (contiguous fp32, 16-byte
 * aligned) and rows an int64 device vector [B] (8-byte aligned): batch row b reads item rows[b]; hidden and d_hidden
 * stay [B][S][D].  Nothing else about a kernel changes - the form is that of ftn_timeproj_form /
 * ftn_timeproj_wide_form / ftn_timeproj_backward_form, and so are the tiles, the K order, the chunks of batch rows, the
 * workspace (ftn_timeproj_backward_workspace) and the reduce kernel - so the result has the bits the unmapped entry
 * gives on the gathered copy seq[rows].  The index is uniform over a workgroup (forward) or over a step of a wave
 * (backward): one scalar load.  An index outside 0 .. n_items - 1 is clamped into that range in the kernel and
 * reported by nobody here (ftn_refit_rows_gather reports it): no index makes a kernel read outside seq.  Arguments
 * are checked before the first launch as by the unmapped entries, plus rows non-null and 8-byte aligned and
 * n_items >= 1. */
int ftn_timeproj_forward_rows(const float* seq_dev, long long n_items, const long long* rows_dev, int B, int L, int D,
                              const float* wt_dev, const float* bt_dev, int S, float* hidden_dev, void* stream);
int ftn_timeproj_wide_forward_rows(const float* seq_dev, long long n_items, const long long* rows_dev, int B, int L,
                                   int D, const float* wt_dev, const float* bt_dev, int S, float* hidden_dev,
                                   void* stream);
int ftn_timeproj_backward_rows(const float* seq_dev, long long n_items, const long long* rows_dev,
                               const float* d_hidden_dev, int B, int L, int S, int D, float* dw_t_dev, float* db_t_dev,
                               void* workspace_dev, size_t workspace_bytes, void* stream);

/* The rest of a cached batch in one launch: batch row b of every output is row rows[b] (clamped as above) of its
 * store.  tail [n_items][tail_floats] (tail_floats = hist N); y, mask, late [n_items][row_floats] (row_floats = S N,
 * >= tail_floats); mask and late are optional (store and output both null).  All fp32, contiguous, 4-byte aligned;
 * a row moves with 16-byte accesses when its length is a multiple of 4 floats and both bases are 16-byte aligned,
 * else float by float.  rows_ok [B] (int64, 8-byte aligned, not overlapping rows) receives the clamped list and
 * status one int32: FTN_REFIT_ROWS_BAD when any rows[b] was outside 0 .. n_items - 1, else 0 - a plain store by one
 * thread, rewritten by every call, no atomics.  As a bare skip word of ftn_refit_update it becomes flag 8: the step
 * is skipped and logged.  One launch of B workgroups, enqueued only. */
#define FTN_REFIT_ROWS_BAD 4
int ftn_refit_rows_gather(const long long* rows_dev, int B, long long n_items, const float* tail_dev, int tail_floats,
                          const float* y_dev, const float* mask_dev_or_null, const float* late_dev_or_null,
                          int row_floats, float* tail_out_dev, float* y_out_dev, float* mask_out_dev_or_null,
                          float* late_out_dev_or_null, long long* rows_ok_dev, int* status_dev, void* stream);

/* The optimiser step of a refit on the device (csrc/refit.hip; additions only: FTN_ABI_VERSION stays 14): clip by
 * the global gradient norm, then AdamW, for n_tensors <= FTN_REFIT_MAX_TENSORS contiguous fp32 tensors of n[i] >= 1
 * elements.  p, m, v are updated in place, g is only read (the clipped gradient is never stored).  Per element, with
 * t' = t + 1 and lr the device word:
 *   norm = sqrt(sum_i sum g^2)             c = max_norm > 0 ? min(1, max_norm / (norm + 1e-6)) : 1        g' = c g
 *   p *= 1 - lr wd        m = b1 m + (1 - b1) g'        v = b2 v + (1 - b2) g'^2
 *   p -= (lr / (1 - b1^t')) m / (sqrt(v) / sqrt(1 - b2^t') + eps)
 * torch's clip_grad_norm_ followed by torch's AdamW.  The sum of squares, c, the decay factor and both bias
 * corrections are fp64, each rounded to fp32 once; element arithmetic is fp32, every operation rounded once (two are
 * fmaf: b1 m + ., b2 v + .), so with c == 1 the result has the bits of the unclipped update.  Partial sums are added
 * in an order that depends on the counts alone - not on the form, not on alignment, not on the run; no atomics.
 * Device words: lr (one float), state[2] = {t, calls} (int32; t counts applied updates, calls every call), n_skip <=
 * FTN_REFIT_MAX_SKIP int32 words passed by address, an optional fp32 loss word, an optional log float [log_cap][4].
 * The update is skipped - p, m, v and t keep every bit - when a skip word is non-zero, the norm is not finite or the
 * loss word is not finite.  calls advances either way, and row calls % log_cap of the log gets (loss, norm before
 * clipping, lr, flags): flag 1 = rate bad, 2 = dispersion bad (bits 0 and 1 of a skip word whose bit in range_mask is
 * clear: a head's `bad` word), 4 = a skip word whose bit in range_mask is set (a block's f16x2 range word) is
 * non-zero, 8 = norm or loss not finite.  Nothing but p, m, v, state, the log row and the workspace is written.
 * Work is dealt in units of 4 consecutive elements of one tensor.  A tensor whose p, g, m and v are all on the 16-byte
 * grid moves whole units with 16-byte accesses and its tail with scalars; any other tensor is moved with scalars
 * (4-byte alignment is required).  ftn_refit_update_form (host-only; the launch dispatches through the same
 * function; misalign_or: per tensor the OR of (address & 15) of its four operands, null for all zero):
 *   bits 0-3    FTN_REFIT_ONE   k_refit_one: one workgroup, norm and update in one launch (up to 2 chunks of 1024
 *                               units: 8192 elements of aligned tensors)
 *               FTN_REFIT_GRID  k_refit_norm + k_refit_apply: a workgroup per chunk writes an fp64 partial to the
 *                               workspace, then every workgroup adds all partials in the same order
 *   bits 4-11   the tensors moved with scalars, one bit each
 *   bits 12-    the number of chunks (at most FTN_REFIT_PARTS_MAX; beyond that the chunk grows)
 * The workspace (ftn_refit_update_workspace bytes, 0 for bad counts; 8-byte aligned; whatever it held before) is read
 * only where this call wrote it; FTN_REFIT_ONE does not touch it.  force_form (0, or a form for tests) overrides the
 * choice where the form can take the counts.  Every argument is checked before the first launch; enqueues only, all
 * launches on the one stream. */
#define FTN_REFIT_MAX_TENSORS 8
#define FTN_REFIT_MAX_SKIP 8
#define FTN_REFIT_PARTS_MAX 1024
#define FTN_REFIT_ONE 1
#define FTN_REFIT_GRID 2
typedef struct FtnRefitArgs {
  float* p[FTN_REFIT_MAX_TENSORS];
  const float* g[FTN_REFIT_MAX_TENSORS];
  float* m[FTN_REFIT_MAX_TENSORS];
  float* v[FTN_REFIT_MAX_TENSORS];
  long long n[FTN_REFIT_MAX_TENSORS];
  int32_t n_tensors, n_skip;
  double beta1, beta2, eps, weight_decay, max_norm;      /* max_norm <= 0: no clip */
  const float* lr_dev;
  int32_t* state_dev;                                     /* {t, calls} */
  const int32_t* skip_dev[FTN_REFIT_MAX_SKIP];
  int32_t range_mask;                                     /* bit k: skip word k is a range word (flag 4) */
  int32_t log_cap;
  const float* loss_dev_or_null;
  float* log_dev_or_null;                                 /* [log_cap][4] */
  void* workspace_dev;  size_t workspace_bytes;
  int32_t force_form, reserved;
} FtnRefitArgs;
int ftn_refit_update_form(int n_tensors, const long long* counts, const int* misalign_or);
size_t ftn_refit_update_workspace(int n_tensors, const long long* counts);
int ftn_refit_update(const FtnRefitArgs* args, void* stream);

/* One step over more than FTN_REFIT_MAX_TENSORS tensors (csrc/refit.hip; additions only: FTN_ABI_VERSION stays 14):
 * n_calls <= FTN_REFIT_LIST_MAX records, each with its own 1 .. 8 tensors, moved by ONE clip-and-AdamW step.  The
 * hyper-parameters, lr, state, skip words, range_mask, loss and log are those of calls[0]; every other record must
 * carry the same values (checked) and the records' own workspace and force_form fields are ignored.  Each record's
 * units are cut into chunks by ftn_refit_update's rule for that record alone; the sum of squares is every record's
 * chunk partials, records ascending, added by ftn_refit_update's total rule over the concatenated list (thread tid
 * adds partials tid, tid + 256, ... ascending, then the workgroup sum).  One decision over the skip and range words,
 * the norm and the loss; one t, one calls word, one log row.  A list of one record IS ftn_refit_update on that record
 * with this workspace: the same launches, the same bits.  With more records: one k_refit_norm launch per record, then
 * one k_refit_apply launch per record, all on the one stream; t is copied beside the partials by the first launch and
 * the words are written by the last, so no launch sees a word another has advanced.  Enqueues only, reads nothing on
 * the host, captureable.  ftn_refit_update_list_workspace: bytes for the counts of all records (counts[c] points at
 * record c's n_tensors[c] counts), 0 for bad counts; 8-byte aligned, whatever it held before. */
#define FTN_REFIT_LIST_MAX 4
size_t ftn_refit_update_list_workspace(int n_calls, const int* n_tensors, const long long* const* counts);
int ftn_refit_update_list(const FtnRefitArgs* calls, int n_calls, void* workspace_dev, size_t workspace_bytes,
                          void* stream);

/* ---- late-bias refit: the late-bias head's forward on stored rows, and its backward (csrc/latefit.hip) ----
 * Additions only: FTN_ABI_VERSION stays 14.
 *
 * The late bias is the one per-series term behind the backbone: for a series row r = (bc, n), c = rows[r][:ctx] the
 * output of context_norm (ftn_context_rows' rows_out, frozen in a refit),
 *   xh = (c - mean) rstd     z = xh gamma + beta     u[s] = W[s] . z + b[s]     late[bc][s][n] = gate[s] u[s]
 * rows [Bc N][ctx], gamma / beta [ctx] (late_bias_norm), W [S][ctx], b [S] (late_bias_head), gate [S]; all contiguous
 * fp32, 4-byte aligned; 1 <= ctx <= 256, S >= 1.  With list_dev (int64 [Bc N], 8-byte aligned) rows is an item store
 * [n_items][ctx] and row r reads item list[r], clamped into 0 .. n_items - 1 in the kernel: the bits of the unmapped
 * call on rows[list] (n_items is ignored without a list).
 *
 * ftn_late_fit_forward (k_late_fit_forward, one wave a row, one launch): late [Bc][S][N], the bits of
 * ftn_context_rows' late_out for the same row and parameters (both kernels share csrc/ftn_ctxrow.h).  A row's outputs
 * are a function of that row and the parameters alone: a NaN row (a bad id's row is all NaN) gives NaN for that row
 * only.
 *
 * ftn_late_backward: d_pre [B][S][N] is the gradient at the rate pre-activation (g_rate sig_mu scale).  Bc == 1: the
 * wide layout, one block of rows serves the batch and Gs[s][n] = sum_b d_pre[b][s][n], b ascending, one chain.
 * Bc == B: batch row b pairs with row block b and Gs = d_pre.  Any other Bc is an error.  With du = gate Gs and
 * dz = du^T W (one chain in s order per k),
 *   dgate[s] = sum_r Gs u     db[s] = sum_r du     dW[s][k] = sum_r du[r][s] z[r][k]
 *   dbeta[k] = sum_r dz[r][k]                      dgamma[k] = sum_r dz[r][k] xh[r][k]
 * rows are frozen: no gradient in them.  Three launches: k_late_bwd_rows (one wave a row: z, du, Gs u, dz, dz xh to
 * the workspace), k_late_bwd_mfma (per chunk of rows: [32 s x 32 k] tiles of [S][ctx + 1] on v_mfma_f32_32x32x2_f32,
 * K = the chunk's rows ascending, column ctx the bias; and the three column sums, one chain in row order),
 * k_late_bwd_reduce (the chunks' partials added in ascending order).  Rows are cut into chunks of 256 (of
 * ceil(R / FTN_LATEFIT_CHUNKS_MAX), made even, beyond 256 chunks).  No atomics, no library GEMM; every sum's order is
 * a function of the sizes alone and every product an exact fp32 fmaf step.  The workspace
 * (ftn_late_backward_workspace bytes, 0 for a bad shape: R (2 S + 3 ctx) + chunks (S (ctx + 1) + S + 2 ctx) floats;
 * 4-byte aligned; whatever it held before) is read only where this call wrote it.  Outputs are written with plain
 * stores and nothing around them is touched.  ftn_late_backward_form (host-only; the launch dispatches through the
 * same function): bits 0-3 FTN_LATEFIT_MFMA (the one form), bits 4-12 the number of chunks. */
#define FTN_LATEFIT_MFMA 1
#define FTN_LATEFIT_CHUNKS_MAX 256
int ftn_late_backward_form(int B, int Bc, int N, int ctx, int S);
size_t ftn_late_backward_workspace(int B, int Bc, int N, int ctx, int S);
int ftn_late_fit_forward(const float* rows_dev, long long n_items, const long long* list_dev_or_null, int Bc, int N,
                         int ctx, int S, const float* ln_g_dev, const float* ln_b_dev, float eps, const float* w_dev,
                         const float* b_dev, const float* gate_dev, float* late_dev, void* stream);
int ftn_late_backward(const float* d_pre_dev, int B, const float* rows_dev, long long n_items,
                      const long long* list_dev_or_null, int Bc, int N, int ctx, int S, const float* ln_g_dev,
                      const float* ln_b_dev, float eps, const float* w_dev, const float* b_dev, const float* gate_dev,
                      float* d_ln_g_dev, float* d_ln_b_dev, float* dw_dev, float* db_dev, float* dgate_dev,
                      void* workspace_dev, size_t workspace_bytes, void* stream);

/* The end of a validated refit epoch on the device (csrc/refit_epoch.hip; additions only: FTN_ABI_VERSION stays 14):
 * the reference's per-epoch bookkeeping (train.py:1536-1572) - validation NLL, ReduceLROnPlateau, best state, early
 * stop - with nothing read on the host.  ftn_refit_epoch_end makes two launches on the one stream.
 *
 * k_epoch_decide (one workgroup) reads acc[n_slots] (the storage ftn_score_fold accumulates into), the scorer's
 * error word, the den_extra word and the state record, and computes in fp64, slots ascending from 0.0,
 *   val_nll   = sum nll_sum / (sum nll_cnt + den_extra)      (0 when the denominator is not > 0)
 *   val_smape = sum smape_sum / sum smape_cnt                (0 when the count is 0)
 * which is the arithmetic of ForecastScorer.result().  Then, in this order:
 *   1. state.stop != 0: the log row gets (NaN, NaN, lr, FTN_EPOCH_AFTER_STOP, 0) and nothing else of the state,
 *      the lr word or the best values changes.
 *   2. epoch += 1; a non-zero error word sets FTN_EPOCH_SCORER_ERR in the row's flags.
 *   3. plateau_patience >= 0 (torch's ReduceLROnPlateau, mode "min", threshold_mode "rel", cooldown 0, eps 1e-8):
 *      val_nll < plateau_best * (1 - threshold) ? (plateau_best = val_nll, num_bad = 0) : num_bad += 1;
 *      num_bad > plateau_patience: new = max(lr * factor, min_lr); lr - new > 1e-8 ? lr = new; num_bad = 0.
 *      All fp64; *lr_dev = (float)lr.  plateau_patience < 0: no schedule, lr is read from *lr_dev and not written.
 *   4. val_nll < best_nll (strict; a NaN is never better): best_nll, best_smape, best_epoch = epoch, patience = 0,
 *      improved = 1; else improved = 0, patience += 1, and patience_limit >= 0 && patience > patience_limit sets
 *      stop = FTN_EPOCH_STOP (as a bare skip word of ftn_refit_update that is flag 8: the step keeps every bit).
 *   5. the log row gets (val_nll, val_smape, lr after, flags, improved).
 * The row is log[state.calls] of double [max_epochs][5] (no row beyond max_epochs is written) and calls advances
 * with every call.  Always, also after the stop: every record of acc, *den_extra_dev and *count_seen_dev_or_null
 * are zeroed, so the next epoch's validation starts clean.  The two sums are each taken by one lane.
 *
 * k_epoch_copy (a grid) then copies src[i] to dst[i] (n[i] >= 1 fp32 each, n_tensors <= FTN_EPOCH_MAX_TENSORS, 0
 * for none; any 4-byte-aligned addresses; no overlap) when state.improved != 0, and leaves every bit of dst
 * otherwise.  ftn_refit_epoch_restore is the same kernel gated on state.best_epoch > 0 (callers pass the store as
 * src).  Work is dealt as by ftn_refit_update: units of 4 elements, chunks of 1024 units (at most
 * FTN_REFIT_PARTS_MAX chunks, beyond that the chunk grows), a workgroup per chunk; a tensor whose src and dst are on
 * the 16-byte grid moves whole units with 16-byte accesses and its tail with scalars, any other tensor with scalars.
 * Plain vector stores, no atomics.  ftn_refit_epoch_form (host-only; the launch dispatches through the same
 * function; misalign_or: per tensor the OR of (address & 15) of src and dst, null for all zero):
 *   bits 0-3    FTN_EPOCH_COPY_VEC  every tensor moves with 16-byte accesses, FTN_EPOCH_COPY_MIXED  some do not
 *   bits 4-11   the tensors moved with scalars, one bit each
 *   bits 12-    the number of chunks
 * Every argument is checked before the first launch; enqueues only. */
#define FTN_EPOCH_MAX_TENSORS 8
#define FTN_EPOCH_STOP 16
#define FTN_EPOCH_AFTER_STOP 16
#define FTN_EPOCH_SCORER_ERR 32
#define FTN_EPOCH_COPY_VEC 1
#define FTN_EPOCH_COPY_MIXED 2
typedef struct FtnEpochState {
  double best_nll, best_smape, plateau_best, lr;          /* +inf, +inf, +inf, the starting rate */
  int32_t epoch, best_epoch, patience, num_bad, stop, improved, calls, reserved;   /* all 0 */
} FtnEpochState;
typedef struct FtnEpochArgs {
  FtnScorePart* acc_dev;  int32_t n_slots, max_epochs;
  const int32_t* err_dev;
  double* den_extra_dev;
  long long* count_seen_dev_or_null;
  FtnEpochState* state_dev;
  float* lr_dev;
  double* log_dev;                                        /* [max_epochs][5] */
  double factor, threshold, min_lr;
  int32_t plateau_patience;                               /* < 0: no plateau schedule */
  int32_t patience_limit;                                 /* < 0: no early stop */
  const float* src[FTN_EPOCH_MAX_TENSORS];
  float* dst[FTN_EPOCH_MAX_TENSORS];
  long long n[FTN_EPOCH_MAX_TENSORS];
  int32_t n_tensors, reserved;
} FtnEpochArgs;
int ftn_refit_epoch_form(int n_tensors, const long long* counts, const int* misalign_or);
int ftn_refit_epoch_end(const FtnEpochArgs* args, void* stream);
int ftn_refit_epoch_restore(const FtnEpochState* state_dev, int n_tensors, const float* const* src, float* const* dst,
                            const long long* counts, void* stream);

/* ---- using the forecast's distribution: NB CDF and quantiles (no counterpart in the reference) -----------
 * These entry points are additions only: no earlier declaration changed, so FTN_ABI_VERSION stays 14.
 *
 * The parameterisation is ftn_score_columns': alpha = disp < eps ? eps : disp, mu = rate < eps ? eps : rate (a NaN
 * stays a NaN), r = 1 / alpha, p = 1 / (1 + alpha mu).  F(k) = I_p(r, k + 1), the regularised incomplete beta
 * function, evaluated in fp64 (continued fraction, modified Lentz) and rounded once.  Operands are fp32 [B][H][N],
 * rows N elements apart, N fastest, each with its own batch stride in elements; outputs are contiguous.
 *
 * ftn_nb_cdf (k_nb_cdf<CPL>): out[b][h][n] = F(floor(yc)), yc = y < 0 ? 0 : y.  NaN where yc, alpha or mu is not
 * finite (the flag stays clear).  floor(yc) >= 2^24, or a continued fraction that used up its iterations, gives NaN
 * and sets FTN_NBQ_RANGE in *flag_dev.  out64_dev (optional): the same values before the rounding to fp32.
 * flag_dev (optional): one int32, OR-ed, never cleared or read here.
 * ftn_nb_quantiles (k_nb_quantile<CPL>): out[i][b][h][n] = the smallest integer k >= 0 with F(k) >= levels_host[i],
 * for Q = 1..FTN_QMAX levels strictly inside (0, 1) in any order (they are passed to the kernel by value).
 * Supported answers are k < 2^24, exact in fp32.  NaN where alpha or mu is not finite (flag clear); an answer
 * >= 2^24 or a search that used up its evaluations gives NaN and sets FTN_NBQ_RANGE in *flag_dev (required).
 * Neither allocates; both enqueue on `stream` only.
 * ftn_nbq_form (host-only; both launches dispatch through the same function):
 *   bit 1      FTN_SHELL_VEC  16-byte loads, four elements per lane (N % 4 == 0, every batch stride a multiple of 4,
 *              misalign_or == 0); otherwise one element per lane
 * misalign_or: the OR of (address & 15) of y, rate, disp and out for ftn_nb_cdf; of rate and disp for
 * ftn_nb_quantiles, which passes y_bstride = 0 and stores 4 bytes at a time. */
#define FTN_QMAX 8
#define FTN_NBQ_RANGE 2
int ftn_nbq_form(int N, long long y_bstride, long long rate_bstride, long long disp_bstride, int misalign_or);
int ftn_nb_cdf(const float* y_dev, long long y_bstride, const float* rate_dev, long long rate_bstride,
               const float* disp_dev, long long disp_bstride, int B, int H, int N, float eps, float* out_dev,
               double* out64_dev, int* flag_dev, void* stream);
int ftn_nb_quantiles(const float* rate_dev, long long rate_bstride, const float* disp_dev, long long disp_bstride,
                     int B, int H, int N, const double* levels_host, int Q, float eps, float* out_dev, int* flag_dev,
                     void* stream);

/* ---- sampling the forecast's distribution (sample.hip) ----
 * ftn_nb_sample (k_nb_sample<CPL>): out[s][b][h][n], s < S, is draw s of the negative binomial (rate, disp) of the
 * element, in the parameterisation, clamps and operand layout of ftn_nb_quantiles: the smallest integer k >= 0 with
 * F(k) >= u, F as ftn_nb_cdf defines it.  The uniforms are the contract:
 *   Philox4x32-10, key = (seed & 0xffffffff, seed >> 32), counter = (e & 0xffffffff, e >> 32, s >> 2, offset) with
 *   e = (b H + h) N + n the logical element index (independent of strides and of the kernel form); draw s takes
 *   output word s & 3; u = (word + 0.5) 2^-32 in fp64.
 * seed_dev (optional): one 64-bit word in device memory, 8-byte aligned, read by the kernel instead of `seed`, so a
 * captured launch can be replayed with another seed.  u_out_dev (optional): the uniforms, fp64 [S][B][H][N].
 * NaN where alpha or mu is not finite (flag clear); an answer >= 2^24 or a search that used up a cap gives NaN and
 * sets FTN_NBQ_RANGE in *flag_dev (required).  S >= 1.  Never allocates; enqueues on `stream` only.
 * ftn_nb_sample_form (host-only; the launch dispatches through the same rule as ftn_nbq_form): bit 1 FTN_SHELL_VEC.
 * misalign_or: the OR of (address & 15) of rate and disp. */
int ftn_nb_sample_form(int N, long long rate_bstride, long long disp_bstride, int misalign_or);
int ftn_nb_sample(const float* rate_dev, long long rate_bstride, const float* disp_dev, long long disp_bstride,
                  int B, int H, int N, int S, unsigned long long seed, const unsigned long long* seed_dev,
                  unsigned offset, float eps, float* out_dev, double* u_out_dev, int* flag_dev, void* stream);

/* ---- summarising sample paths (paths.hip) ----
 * Additions only, as the three sections above: FTN_ABI_VERSION stays 14.
 *
 * ftn_path_summary (k_path_reg<PP,CPL> / k_path_lds<CPL>): samples is fp32 [P][B][H][N], rows N elements apart, N
 * fastest, with a path stride and a batch stride in elements; y (optional) fp32 [B][H][N] with its own batch stride;
 * outputs are contiguous.  H % window == 0, H' = H / window, 1 <= P <= FTN_PATHS_MAX; sample addresses are formed in
 * 64 bits, B H' N must fit an int32.  Per output element (b, h', n):
 *   v[p]  the reduce over j = 0 .. window - 1, ascending, of samples[p][b][h' window + j][n]: FTN_PATH_SUM accumulates
 *         in fp64 and rounds once to fp32; FTN_PATH_MAX is the maximum, a NaN staying as in torch.amax.  yw is the
 *         same reduce of y.
 *   x(1) <= .. <= x(P)  v sorted ascending in torch.sort's value order, NaN after +inf.  Values are only permuted:
 *         the sorted column holds the bits of v, except that every NaN comes out as the quiet NaN 0x7FC00000 and that
 *         -0 sorts before +0 (torch leaves their order to the input).
 *   q_out[i]  = x(ranks_host[i]), Q = 0 .. FTN_QMAX ranks in 1 .. P, passed to the kernel by value
 *   mean_out  = (sum_p x(p)) / P: the sum in fp64, one fp64 division, one rounding to fp32
 *   crps_out  = (A P - G) / (P P), A = sum_p |x(p) - yw|, G = sum_{i=1..P} (2 i - P - 1) x(i), both sums in fp64 (every
 *         product exact), then one fp64 product, difference and division and one rounding to fp32.  This is the
 *         ensemble estimator (1/P) sum_p |v[p] - yw| - (1/(2 P P)) sum_p sum_p' |v[p] - v[p']|; for integer-valued
 *         samples A, G and the numerator are exact and the result is the correctly rounded quotient.  A value that is
 *         not finite gives what IEEE arithmetic gives from these formulas (NaN).
 *   sorted_out[p] = x(p + 1)
 * The sums run in ascending rank; above 64 paths they are R = 256 / T interleaved partial sums (ranks r, r + R, ..)
 * added in ascending r, so their order is a function of P alone.  An element's result does not depend on the grid,
 * on the load width or on which other elements share the call.  Anything outside these rules (a rank outside 1 .. P,
 * crps_out without y, Q > FTN_QMAX, q_out null with Q > 0, no output at all, a stride below its span) is a negative
 * return with ftn_last_error set and nothing launched.  Never allocates, never synchronises; enqueues one kernel on
 * `stream`; no atomics.
 * ftn_path_summary_form (host-only; the launch dispatches through the same function):
 *   bit 1       FTN_SHELL_VEC  16-byte loads (and stores in the register form), four columns per lane: N % 4 == 0,
 *               every stride a multiple of 4, misalign_or == 0, and the padded P at most 16 or above 64 (four columns
 *               of 32 or 64 keys do not fit a lane's registers); otherwise 4-byte accesses, one column per lane.
 *               Either way consecutive n lie on consecutive lanes.
 *   bit 4       FTN_PATH_LDS   k_path_lds (padded P above 64): a workgroup sorts a tile of T columns in LDS;
 *               otherwise k_path_reg: a lane sorts its columns in registers
 *   bits 8-19   the padded P: the power of two >= max(P, 2), the size of the bitonic network
 *   bits 20-27  T, the columns of an LDS tile (padded P x T x 4 bytes <= 64 KiB, T <= 64), 0 in the register form
 * misalign_or: the OR of (address & 15) of samples, y and every output of the call. */
#define FTN_PATHS_MAX 1024
#define FTN_PATH_SUM 0
#define FTN_PATH_MAX 1
#define FTN_PATH_LDS 16
int ftn_path_summary_form(int P, int N, int window, long long p_stride, long long b_stride, long long y_bstride,
                          int misalign_or);
int ftn_path_summary(const float* samples_dev, long long p_stride, long long b_stride, int P, int B, int H, int N,
                     int window, int reduce, const float* y_dev, long long y_bstride, const int* ranks_host, int Q,
                     float* q_out_dev, float* mean_out_dev, float* crps_out_dev, float* sorted_out_dev, void* stream);

/* ---- series groups: segmented sums along the series axis (groups.hip) ----
 * Additions only, as the four sections above: FTN_ABI_VERSION stays 14.
 *
 * ftn_group_sum (k_group_sum<VEC>): x is fp32 [rows][N], rows row_stride >= N elements apart; out is fp32 [rows][G],
 * contiguous.  The groups are member lists in CSR form, int32, on the device:
 *   order    [M]      series indices in 0 .. N - 1
 *   offsets  [G + 1]  non-decreasing, offsets[0] = 0, offsets[G] = M
 * and group g's members are order[offsets[g] .. offsets[g + 1]), in that order.  A series may belong to no group, to
 * one or to several; an empty group is allowed.  offsets_host is the same G + 1 words in host memory: the call
 * validates them and sizes the launch from them, so nothing is read back.  For a row x[0 .. N) and a group of m
 * members i_0 .. i_{m-1}:
 *   1. the members are split into chunks of FTN_GROUP_CHUNK = 32 consecutive members, the last possibly shorter;
 *   2. a chunk's sum is formed in fp64, left to right, starting from +0.0;
 *   3. the chunk sums are added in ascending chunk order in fp64;
 *   4. the total is rounded once to fp32.
 * An empty group gives +0.  NaN and inf behave as IEEE addition gives them and reach only the groups that hold the
 * element.  A group's result is a function of its member list and of the row alone: not of the number of rows, of
 * the other groups, of the load width or of the grid.  For integer-valued x whose totals stay below 2^24 the result
 * is exact.  No atomics; no loop bound depends on the data, only on the CSR.  What the kernel reads from the device
 * CSR is clamped: offsets to 0 .. M, and a member outside 0 .. N - 1 contributes +0 and touches no memory.
 * Limits, checked before the launch: 1 <= N <= FTN_GROUP_NMAX, 1 <= G <= FTN_GROUP_GMAX, at most FTN_GROUP_CHUNKS_MAX
 * chunks over all groups (a group of m members has ceil(m / 32)); rows >= 1, rows row_stride and rows G formed in 64
 * bits; row_stride >= N; offsets_host monotone from 0 to M; every pointer non-null (order may be null when M = 0)
 * and 4-byte aligned.  Anything else is a negative return with ftn_last_error set and nothing launched.  Never
 * allocates, never synchronises; enqueues one kernel on `stream`.
 * A workgroup takes tiles of T rows: it stages each row into LDS (element i at word i + (i >> 5) of its row, so the
 * 32 lanes that walk 32 chunks of consecutive series hit 32 banks), a work item (row, chunk) adds its chunk out of
 * LDS, and after a barrier one thread per (row, group) adds that group's chunk sums and stores, G fastest.
 * ftn_group_sum_form (host-only; the launch dispatches through the same function):
 *   bit 1      FTN_SHELL_VEC  16-byte loads of x: N % 4 == 0, row_stride % 4 == 0 and misalign_or == 0; otherwise
 *              4-byte loads.  Either way consecutive elements lie on consecutive lanes.
 *   bits 8-15  T, the rows of a tile: a row takes 4 (N + N / 32 + 1) + 8 n_chunks bytes of LDS (the staged row, one
 *              zero word, the fp64 chunk sums); T = FTN_GROUP_TILE_BYTES / that, at most FTN_GROUP_TILE_ROWS and at
 *              least 1 (within the limits one row takes at most 50180 bytes).
 * misalign_or: (address of x) & 15. */
#define FTN_GROUP_CHUNK 32
#define FTN_GROUP_NMAX 8192
#define FTN_GROUP_GMAX 2048
#define FTN_GROUP_CHUNKS_MAX 2048
#define FTN_GROUP_TILE_BYTES 32768
#define FTN_GROUP_TILE_ROWS 64
int ftn_group_sum_form(int N, long long row_stride, int misalign_or, int n_chunks);
int ftn_group_sum(const float* x_dev, long long rows, int N, long long row_stride, const int* order_dev,
                  const int* offsets_dev, const int* offsets_host, int G, int M, float* out_dev, void* stream);

/* ---- series groups along an axis that is not the fastest one (groups_rows.hip) ----
 * Additions only: FTN_ABI_VERSION stays 14.
 *
 * ftn_group_sum_rows (k_group_sum_rows<VEC>): x is fp32 [outer][S][inner], element (o, s, i) at
 * x + o outer_stride + s member_stride + i (inner contiguous); out is fp32 [outer][G][inner], contiguous.  The CSR
 * (order [M] with members in 0 .. S - 1, offsets [G + 1], offsets_host) is that of ftn_group_sum.  For every (o, i)
 * the column x[o][.][i] is summed per group by rules 1-4 of ftn_group_sum, so the result equals ftn_group_sum on the
 * transposed copy bit for bit, and its guarantees carry over: an empty group gives +0; NaN and inf reach only the
 * groups that hold them; integer totals below 2^24 are exact; a group's result is a function of its member list and
 * of its column alone - not of outer, of inner, of where the column falls in a tile, of the load width, of the grid
 * or of the other groups.  No atomics; no loop bound depends on the data, only on the CSR.  What the kernel reads
 * from the device CSR is clamped: offsets to 0 .. M, and a member outside 0 .. S - 1 contributes +0 and touches no
 * memory.
 * Limits, checked before the launch: 1 <= S < 2^31 (no FTN_GROUP_NMAX: the member axis is walked, not staged),
 * 1 <= G <= FTN_GROUP_GMAX, at most FTN_GROUP_CHUNKS_MAX chunks; outer >= 1, inner >= 1; member_stride >= inner;
 * outer_stride >= S member_stride unless outer == 1 (then it is ignored); S member_stride, outer outer_stride and
 * outer G inner formed in 64 bits and rejected on overflow; offsets_host monotone from 0 to M; every pointer non-null
 * (order may be null when M = 0) and 4-byte aligned.  Anything else is a negative return with ftn_last_error set and
 * nothing launched.  Never allocates, never synchronises; enqueues one kernel on `stream`.
 * A workgroup takes tiles of one o and TI consecutive inner columns, and a tile takes the chunks in passes of CP: a
 * work item (chunk, column), columns fastest along the lanes, walks its chunk's members with an fp64 accumulator and
 * leaves the chunk sum in LDS ([CP][TI] fp64); after a barrier one thread per (group, column) adds that group's chunk
 * sums of the pass in ascending order and stores, columns fastest; the one group that runs past the end of a pass
 * hands its fp64 running sum to the next pass through LDS - the same chain of additions.
 * ftn_group_sum_rows_form (host-only; the launch dispatches through the same function):
 *   bit 1       FTN_SHELL_VEC  16-byte loads of x and stores of out along inner, an item taking 4 columns:
 *               inner % 4 == 0, member_stride % 4 == 0, outer_stride % 4 == 0 and misalign_or == 0; otherwise 4-byte
 *               loads and stores.  Either way consecutive columns lie on consecutive lanes.
 *   bits 8-15   TI, the inner columns of a tile: min(inner, FTN_GROUP_TILE_COLS), rounded down to a multiple of 4
 *               when it is 4 or more - a member row's columns are one contiguous run, the whole row up to 64.
 *   bits 16-27  the passes of a tile: ceil(n_chunks / CP), at least 1, with CP = FTN_GROUP_TILE_BYTES / (8 TI) chunks a
 *               pass (the chunk sums of a pass stay within FTN_GROUP_TILE_BYTES of LDS; 512 chunks of 8 columns, 146
 *               of 28, 64 of 64).
 * misalign_or: ((address of x) | (address of out)) & 15.  outer_stride: 0 when outer == 1. */
#define FTN_GROUP_TILE_COLS 64
int ftn_group_sum_rows_form(long long inner, long long member_stride, long long outer_stride, int misalign_or,
                            int n_chunks);
int ftn_group_sum_rows(const float* x_dev, long long outer, int S, long long inner, long long outer_stride,
                       long long member_stride, const int* order_dev, const int* offsets_dev, const int* offsets_host,
                       int G, int M, float* out_dev, void* stream);

/* ---- context front end (csrc/context.hip) ----
 * Additions only: FTN_ABI_VERSION stays 14.
 *
 * What TimesNet.forward computes from the series rows before the value embedding and the heads see it (:1883-2020,
 * :2080-2090), as three launches.  Plain fp32 on the VALU: every sum is one chain of FMAs in index order from +0, or
 * a fixed tree of such chains whose shape depends on the sizes alone.  No atomics, no workspace, no allocation, no
 * synchronisation: each entry enqueues one kernel on `stream`.  A bad argument is a negative return with
 * ftn_last_error set (the entry's name first) and nothing launched.  Every fp32 operand is 4-byte aligned unless
 * stated otherwise.
 *
 * ftn_context_rows (k_context_rows): rows = Bc N, one wave a row (bc, n), ctx = Ws + Ed.
 *   s     = static_norm(W_s static[bc][n] + b_s)         W_s [Ws][F]; no norm when sn_g is null; absent when Ws == 0
 *   e     = E[ids[bc][n]]                                E [V][Ed], ids int64 (8-byte aligned); absent when Ed == 0
 *   c     = context_norm(cat(s, e))                      -> rows_out [rows][ctx]
 *   coeff = W_c c + b_c                                  W_c [R][ctx] -> coeff_out [rows][R]
 *   cbias = w_p c + b_p                                  -> cbias_out [rows]
 *   late  = gate[s] (W_l late_bias_norm(c) + b_l)[s]     W_l [steps][ctx] -> late_out [Bc][steps][N]
 * Each output is optional (at least one).  static row (bc, n) is at static + bc static_bstride + n F, the id at
 * ids + bc ids_bstride + n; both strides are ignored when Bc == 1 and may be 0 (one [N] block for every bc).  The
 * LayerNorms are torch's: the mean, the biased variance of the centred values, 1 / sqrt(var + eps), gamma, beta.
 * An id outside [0, V) reads nothing from the table: every output of that row is NaN, no other row changes.
 * A row's outputs are a function of that row's inputs and the parameters alone - the same bits whatever Bc and N
 * are and whichever rows share the call.  Limits: ctx, F, Ws, Ed <= 256, R <= 32, any steps >= 1.
 * ftn_context_rows_form (host-only): bits 0-3 ceil(ctx / 64), the slots of a lane's share of a context vector;
 * bits 4-7 ceil(Ws / 64); bits 8-15 min(ceil(steps / 64), 255), the passes of the late head.
 *
 * ftn_context_through_weight: the contraction over series of the two context terms with the value weight w [D][N]
 * (row stride w_rstride >= N: a column slice is fine),
 *   q_coeff[bc][r][d] = sum_n coeff[bc][n][r] w[d][n]     q_bias[bc][d] = sum_n cbias[bc][n] w[d][n]
 * coeff [Bc][N][R], cbias [Bc][N], q_coeff [Bc][R][D], q_bias [Bc][D], all contiguous; either output optional.
 * N <= 64 (k_through_small): one chain in n order.  N > 64 (k_through_chunks): chunks of 64 series, chunk c belongs
 * to part c mod 4, a part adds its chunks' products in n order in one chain, and the result is
 * (p0 + p1) + (p2 + p3).  A batch row's bits do not depend on Bc.  D a multiple of 4, <= 512; R <= 32;
 * Bc <= 65535 when N > 64.
 *
 * ftn_embed_add (k_embed_add<NO, VEC>): the `add` operand of the embedding entry points, [Ba][L][D] contiguous,
 * 16-byte aligned, one wave a row, the terms applied left to right:
 *   aux = pos[l] (+ (mark[b][l] W_t^T + b_t));  aux = gate * LayerNorm(aux) when aux_g is given ("decoupled")
 *   t   = aux + b_v                             (this part only when pos is given)
 *   t   = t + scale (sum_r basisc[l][r] q_coeff[b][r])     (when q_coeff is given; scale is read from the device)
 *   add = t + q_bias[b]                                      (when q_bias is given)
 * pos [L][D]; mark row (b, l) at mark + b mark_bstride + l T (mark_bstride may be 0); W_t [D][T], T <= 64; basisc
 * [L][R]; q_coeff / q_bias batch strides in elements (0: shared by the batch).  D a multiple of 4, <= 512.
 * ftn_embed_add_form (host-only; the launch dispatches through the same function):
 *   bit 1      FTN_SHELL_VEC  16-byte loads of the row-shaped operands (pos, b_t, gate, aux gamma / beta, b_v,
 *                             q_coeff, q_bias): both batch strides % 4 == 0 and misalign_or == 0 (the OR of those
 *                             operands' byte offsets from a 16-byte boundary); otherwise 4-byte loads, same arithmetic
 *   bits 4-7   NO: 4-column groups of a lane (1 for D <= 256, else 2) */
typedef struct FtnContextParams {
  const float* w_s;  const float* b_s;                    /* static_proj */
  const float* sn_g; const float* sn_b;                   /* static_norm (null: none) */
  const float* emb;                                       /* series_embedding table */
  const float* cn_g; const float* cn_b;                   /* context_norm */
  const float* w_c;  const float* b_c;                    /* context_coeff */
  const float* w_p;  const float* b_p;                    /* context_proj */
  const float* ln_g; const float* ln_b;                   /* late_bias_norm */
  const float* w_l;  const float* b_l; const float* gate; /* late_bias_head, late_bias_gate [steps] */
  float sn_eps, cn_eps, ln_eps;
  int32_t F, Ws, Ed, V, R, steps;
  int32_t reserved;
} FtnContextParams;

typedef struct FtnEmbedAddParams {
  const float* pos;                                       /* PositionalEmbedding table [L][D] (null: no epilogue part) */
  const float* w_t;  const float* b_t;                    /* temporal_embedding */
  const float* aux_g; const float* aux_b; const float* gate;   /* aux_norm and the gate [D] (null: not "decoupled") */
  const float* b_v;                                       /* value_embedding bias */
  const float* basisc; const float* scale;                /* centred DCT basis [L][R], temporal_context.scale [1] */
  float aux_eps;
  int32_t T;
} FtnEmbedAddParams;

int ftn_context_rows_form(int F, int Ws, int Ed, int R, int steps);
int ftn_context_rows(const FtnContextParams* params, const float* static_dev_or_null, long long static_bstride,
                     const long long* ids_dev_or_null, long long ids_bstride, int Bc, int N,
                     float* rows_out_or_null, float* coeff_out_or_null, float* cbias_out_or_null,
                     float* late_out_or_null, void* stream);
int ftn_context_through_weight(const float* coeff_dev_or_null, const float* cbias_dev_or_null, int Bc, int N, int R,
                               const float* w_dev, long long w_rstride, int D, float* q_coeff_out_or_null,
                               float* q_bias_out_or_null, void* stream);
int ftn_embed_add_form(int D, long long q_coeff_bstride, long long q_bias_bstride, int misalign_or);
int ftn_embed_add(const FtnEmbedAddParams* params, const float* mark_dev_or_null, long long mark_bstride,
                  const float* q_coeff_dev_or_null, long long q_coeff_bstride, int R,
                  const float* q_bias_dev_or_null, long long q_bias_bstride, int Ba, int L, int D, float* out_dev,
                  void* stream);

/* ---- device windows: the batches of a rolling-origin backtest (csrc/windows.hip) ----
 * Additions only: FTN_ABI_VERSION stays 14.
 *
 * The wide table of a validation fold lives on the device once: X fp32 [T][N] (values), M fp32 [T][N] (validity,
 * optional), marks fp32 [T][F] (time features, optional), statics fp32 [N][Fs] and ids int64 [N] (optional), and
 * starts int32 [W], the first row s_w of every window (a window is rows s_w .. s_w + L + H - 1).  X, M and marks have
 * row strides in elements (>= N, >= N, >= F), so a fold (a row slice) and a subset of series (a column slice) are
 * passed in place; statics and ids are contiguous.
 *
 * ftn_window_batch (k_window_batch) enqueues ONE kernel on `stream` that writes the pieces of items
 * item0 .. item0 + count - 1 into rows r = 0 .. count - 1 of the outputs.  It never allocates and never
 * synchronises.  Every output is optional (a null pointer; at least one is given) and contiguous, and every value is
 * a bit copy: NaN payloads, -0 and inf arrive unchanged.
 *   FTN_WIN_SERIES  one series of one window per item, the order of the reference's SlidingWindowDataset
 *                   (data/dataset.py:173-204): item k is window k / N, series i = k % N; with s = starts[k / N],
 *                   e = s + L and r = k - item0
 *                     x      [count][L]      x[r][l]         = X[s + l][i]
 *                     y      [count][H]      y[r][h]         = X[e + h][i]
 *                     mask   [count][H]      mask[r][h]      = M[e + h][i], or 1.0f when M is null (stored, not read)
 *                     x_mark [count][L][F]   x_mark[r][l][f] = marks[s + l][f]
 *                     y_mark [count][H][F]   y_mark[r][h][f] = marks[e + h][f]
 *                     static [count][Fs]     static[r][:]    = statics[i][:]
 *                     id     [count]         id[r]           = ids[i]
 *                   A batch may start and end inside a window: it then takes a partial run of series of its first
 *                   and last window.  item0 + count <= W N.
 *   FTN_WIN_WIDE    one window per item (this project's [B][L][N] layout): item k is window k, s = starts[k]
 *                     x [count][L][N]  x[r][l][n] = X[s + l][n];  y and mask [count][H][N] from rows e + h likewise;
 *                     x_mark and y_mark as above.  Statics and ids are shared by the batch and not copied: asking
 *                     for them is an error.  item0 + count <= W.
 * starts_host is the same W words in host memory: the call validates them (0 <= s, s + L + H <= T) and sizes nothing
 * from device data - the arrangement of offsets_host in ftn_group_sum.  What the kernel reads from the device copy is
 * clamped to 0 .. T - L - H, so nothing outside the tables is ever read, not by a masked-off lane either, and
 * nothing outside rows 0 .. count - 1 of the outputs is written.
 * Limits, checked before the launch: 1 <= N, 1 <= L, 1 <= H, 0 <= F, 0 <= Fs, (L + H) max(N, F, Fs) < 2^31 (the words
 * of one item's piece are counted in 32 bits), W >= 1, T >= L + H, count >= 1, 0 <= item0, item0 + count within the
 * items; T times every row stride and count times the words of an item's piece formed in 64 bits and rejected on
 * overflow; row strides as above; marks only with F >= 1 and statics only with Fs >= 1; x_mark / y_mark only with
 * marks, static only with statics, id only with ids; X, starts and starts_host non-null; every pointer 4-byte
 * aligned, ids and id 8-byte.  Anything else is a negative return with ftn_last_error set and nothing launched.
 * No grid dimension carries count, W, L or T: a workgroup of 256 threads strides over the work units of all pieces
 * (at most 4096 workgroups), and every address is formed in 64 bits.
 * The kernel.  x, y and mask of FTN_WIN_SERIES are a transposition: a tile is (one window, FTN_WIN_TILE_SERIES = 64
 * consecutive series, FTN_WIN_TILE_STEPS = 32 consecutive time steps), read along the series - the contiguous
 * direction of the table - and written along time - the contiguous direction of an item row; consecutive series are
 * consecutive output rows, so a tile that holds all of a row's steps is one contiguous run of the output.  The tile
 * passes through LDS with a row stride of 65 words, which keeps both directions off shared banks.  Everything else
 * (FTN_WIN_WIDE, the marks, statics, ids) is row copies in units of 1024 consecutive output words.
 * ftn_window_batch_form (host-only; the launch dispatches through the same function; reads the dimensions, the row
 * strides, which pointers are null and the low 4 bits of the addresses - starts, T, W, item0 and count are ignored):
 *   bits 0-4    the pieces x, y, mask, x_mark, y_mark that move 16 bytes a lane (a bit is 0 for a piece that is not
 *               requested); the others move 4 bytes a lane.  Same bits either way.  For a piece with table `tab`
 *               (X, M or marks; none for mask when M is null), row stride `stride` and output `out`:
 *                 x, y, mask of FTN_WIN_SERIES  N % 4 == 0, J % 4 == 0 (J = L for x, H for y and mask),
 *                                               stride % 4 == 0, ((tab | out) & 15) == 0: quads of series are
 *                                               loaded, quads of time steps stored
 *                 x, y, mask of FTN_WIN_WIDE    N % 4 == 0, stride % 4 == 0, ((tab | out) & 15) == 0
 *                 x_mark, y_mark                F % 4 == 0, stride % 4 == 0, ((tab | out) & 15) == 0
 *               static and id always move 4 bytes a lane.
 *   bits 8-15   FTN_WIN_TILE_SERIES and bits 16-23 FTN_WIN_TILE_STEPS when x, y or mask of FTN_WIN_SERIES is
 *               requested (the tile of the transposition), else 0. */
#define FTN_WIN_SERIES 0
#define FTN_WIN_WIDE 1
#define FTN_WIN_TILE_SERIES 64
#define FTN_WIN_TILE_STEPS 32
typedef struct FtnWindowArgs {
  const float* X;        long long x_stride;              /* [T][N] values */
  const float* M;        long long m_stride;              /* [T][N] validity (null: a mask of ones) */
  const float* marks;    long long marks_stride;          /* [T][F] time features (null: none) */
  const float* statics;                                   /* [N][Fs] (null: none) */
  const long long* ids;                                   /* [N] (null: none) */
  const int32_t* starts; const int32_t* starts_host;      /* [W] window start rows, on the device and on the host */
  long long T, item0, count;
  int32_t N, L, H, F, Fs, W, layout, reserved;
  float* x; float* y; float* mask; float* x_mark; float* y_mark; float* static_out;   /* outputs, each optional */
  long long* id_out;
} FtnWindowArgs;
int ftn_window_batch_form(const FtnWindowArgs* args);
int ftn_window_batch(const FtnWindowArgs* args, void* stream);

/* ---- training windows: shuffled epochs, time shift and noise (csrc/windows_gather.hip) ----
 * Additions only: FTN_ABI_VERSION stays 14.
 *
 * The reference trains on DataLoader(SlidingWindowDataset(..., augment), shuffle=True, drop_last=True) (train.py:933,
 * data/dataset.py:181-193).  Here an epoch is a pure function of (seed, epoch) on the project's own generator,
 * Philox4x32-10 as in ftn_nb_sample: key = (seed & 0xffffffff, seed >> 32), counter = (k & 0xffffffff, k >> 32, q,
 * epoch << 2 | purpose), k the item's global index, 0 <= epoch < 2^30, output words (x, y, z, w).
 *   order  (purpose 0, q = 0)  key64(k) = the signed int64 with bits (x << 32) | y; the epoch's order is the stable
 *          ascending argsort of key64(0 .. n_items - 1).  ftn_epoch_keys writes key64(k), k < n, in one launch; the
 *          sort is the caller's, once per epoch.
 *   shift  (purpose 1, q = 0, ts >= 1)  delta = ((uint64) x (2 ts + 1) >> 32) - ts; the item's start row is
 *          clamp(starts[w] + delta, 0, T - L - H) and serves x, y, mask, x_mark and y_mark together.  ts = 0: no shift
 *          and no generator call.
 *   noise  (purpose 2, noise_std > 0)  j = the element's index inside the item's x (l in FTN_WIN_SERIES, l N + n in
 *          FTN_WIN_WIDE), q = j >> 2; words (x, y) serve lanes j & 3 = 0, 1 and (z, w) lanes 2, 3: for a pair (a, b),
 *          u1 = (a + 0.5) 2^-32, u2 = (b + 0.5) 2^-32, r = sqrt(-2 ln u1), the even lane gets z = r cos(2 pi u2) and
 *          the odd lane z = r sin(2 pi u2), all in fp64; x_out = fp32(double(x) + noise_std z), the product and the
 *          sum rounded once each.  Only x is touched; noise_std = 0 leaves it a bit copy.
 *
 * ftn_window_gather (k_window_gather) enqueues ONE kernel on `stream` that writes the pieces of the items
 * items[0 .. count - 1] (int64 on the device, global indices) into rows 0 .. count - 1 of the outputs of `w`, which
 * are those of ftn_window_batch with the same shapes.  w.item0 is item_lo, the global index of this part's first
 * item; a row whose item is outside item_lo .. item_lo + (W N | W) - 1 is left untouched and nothing is read for it,
 * so a batch over several parts is one launch per part into the same outputs.  It never allocates and never
 * synchronises; the items are not validated on the host and need not be.
 *   FTN_WIN_SERIES  x, y and mask are read from the series-major copies XT [N][xt_stride] and MT [N][mt_stride]
 *                   (row strides >= T; XT[i][t] = X[t][i]; MT null: a mask of ones): an item's x and y are the
 *                   contiguous run XT[i][s .. s + L + H).  w.X and w.M are checked like ftn_window_batch's and not
 *                   read.  statics and ids as in ftn_window_batch.
 *   FTN_WIN_WIDE    x, y and mask are rows of w.X and w.M; XT and MT are ignored.
 *   the marks       rows of w.marks in both layouts.
 * The kernel is row copies: units of 1024 consecutive output words over at most 4096 workgroups of 256 threads, one
 * indirection per row (the rows of a unit get their series and shifted start once, in LDS), consecutive lanes on
 * consecutive words of a table row, 4 bytes a lane; every address is formed in 64 bits and no grid dimension carries
 * count, L or T.  There is one kernel form.
 * Limits, checked before the launch: those of ftn_window_batch on `w` (its item range aside), item_lo >= 0,
 * count >= 1, items non-null and 8-byte aligned, ts >= 0 (so 2 ts + 1 < 2^32), noise_std finite and >= 0,
 * epoch < 2^30, XT given with xt_stride >= T in FTN_WIN_SERIES.  Anything else is a negative return with
 * ftn_last_error set and nothing launched. */
typedef struct FtnWindowGatherArgs {
  FtnWindowArgs w;                                        /* tables, starts, dimensions, outputs; item0 = item_lo */
  const float* XT;       long long xt_stride;             /* [N][xt_stride] series-major values (FTN_WIN_SERIES) */
  const float* MT;       long long mt_stride;             /* [N][mt_stride] series-major validity (null: ones) */
  const long long* items;                                 /* [count] global item indices, on the device */
  unsigned long long seed;
  double noise_std;
  uint32_t epoch; int32_t ts;
} FtnWindowGatherArgs;
int ftn_epoch_keys(long long n, unsigned long long seed, unsigned epoch, long long* keys_dev, void* stream);
int ftn_window_gather(const FtnWindowGatherArgs* args, void* stream);

/* ---- table preparation: static features, scalers, their transform and inverse (csrc/table.hip) ----
 * Additions only: FTN_ABI_VERSION stays 14.
 *
 * What the reference does to the wide table X fp32 [T][N] (validity M fp32 [T][N], optional) before the loader -
 * compute_series_features (utils/static_features.py:17-103), fit_series_scaler (utils/io.py:548-597),
 * _transform_dataframe (train.py:569-592) - and to the forecast after the model - inverse_transform and the clip at 0
 * (utils/io.py:600-621, predict.py:959-961).  X and M have row strides in elements (>= N): a fold (a row slice) and a
 * subset of series (a column slice) are passed in place.  No entry allocates, none synchronises, every limit is
 * checked before the first launch (a violation is a negative return with ftn_last_error set and nothing launched),
 * every address is formed in 64 bits, no grid dimension carries N or T (workgroups of 256 threads stride over the
 * work units, at most 4096 of them), there are no floating-point atomics, and the bits do not depend on the run.
 * A validity value counts when it is > 0; the value of an element that does not count is loaded and discarded.
 *
 * ftn_table_moments: per column over rows 0 .. T - 1, the statistics stats fp64 [6][N], or [12][N] with FTN_TAB_DIFF:
 *   row 0 count   the elements that count (all T without FTN_TAB_MASK; M is ignored then and may be null)
 *   row 1 sum     their fp64 sum (with FTN_TAB_CLIP every value is read as v < 0 ? 0 : v; nothing is written back)
 *   row 2 mean    fp32(sum / max(count, 1)), rounded once; NaN when the sum is not finite
 *   row 3 css     sum of double(d)^2, d = fp32(v - mean) formed in fp32, squares and sums in fp64
 *   row 4 / 5     min and max (fp32 values; a NaN that counts is kept, as numpy keeps it; +inf / -inf when count = 0)
 *   rows 6 - 11   the same six of the first differences fp32(v[t] - v[t-1]), t = 1 .. T - 1, where both rows count
 * Order: a thread owns a column (the 16-byte form: four columns with one 16-byte load when N % 4 == 0, the row strides
 * are multiples of 4 and the tables are 16-byte aligned; same bits either way) and a block of rb consecutive rows,
 * rb = 32 doubled until at most FTN_TAB_PARTIALS_MAX = 32 blocks cover T, and adds its rows ascending; the blocks'
 * partials are added ascending.  Two passes over the table (the centred sums need the mean), a launch between them
 * that finishes the means once a column, and a combining launch.
 * workspace: ftn_table_moments_bytes(T, N), 8-byte aligned, contents irrelevant before and after.
 *
 * ftn_table_twiddle_bytes / ftn_table_twiddle_init: the table of T twiddles (cos, sin)(2 pi m / T), m = 0 .. T - 1,
 * evaluated in fp64 on the exactly reduced argument and rounded to fp32 - the analogue of ftn_dft_table_*.
 *
 * ftn_table_spectrum: with d[t][n] = (M null or M[t][n] > 0) ? fp32(X[t][n] - mean[n]) : 0 and, for f = 1 .. F =
 * floor(T / 2), ph = 2 pi ((f t) mod T) / T, re = sum_t d cos(ph), im = sum_t d sin(ph), P[f][n] = re^2 + im^2, per
 * column: f_peak int32 [N], the lowest f that attains the maximum of P (0 when T = 1); peak fp32 [N] = P[f_peak];
 * total fp32 [N] = the fp64 sum of the fp32 P[f] rounded once (0, 0 when T = 1; a NaN total makes peak NaN).
 * The sums run on v_mfma_f32_32x32x2_f32 with the twiddles as A and d as B (k_spectrum's convention); a workgroup
 * owns FTN_TAB_SPEC_COLS = 64 columns and FTN_TAB_SPEC_BINS = 128 bins and stages d through LDS in chunks of
 * FTN_TAB_SPEC_CHUNK = 128 rows; the phase index is carried exactly as m += 2 f mod T.  P is not written unless
 * power_out fp32 [F][N] (contiguous, optional) is given.  The peaks and totals of the bin blocks pass through the
 * workspace (ftn_table_spectrum_bytes(T, N), 8-byte aligned) and are combined ascending.  1 <= T <= 65536; a larger
 * T is refused.  `twiddle` is the table of ftn_table_twiddle_init for this T; mean fp32 [N].
 *
 * ftn_table_features: the five features out fp32 [N][5] (mean, std, diff_std, seasonal_strength, dominant_period)
 * from the [12][N] statistics of a FTN_TAB_MASK | FTN_TAB_DIFF call and the three spectrum outputs:
 * std = sqrt(fp32(css / max(count, 1))), seasonal_strength = peak / max(total, 1e-6) (numpy's maximum: a NaN stays),
 * dominant_period = total > 1e-6 ? fp32(double(T) / f_peak) : 0; diff_std, seasonal_strength and dominant_period are
 * 0 when T = 1; a column whose mean is NaN gives (NaN, NaN, NaN, NaN, 0).
 *
 * ftn_table_scaler: loc fp32 [N], scale fp32 [N] and the reference's pairs fp32 [2][N] from the [6][N] statistics
 * of a call without FTN_TAB_MASK.  FTN_TAB_ZSCORE: pairs (mean, sd), sd = sqrt(fp32(css / count)), sd < eps -> 1;
 * FTN_TAB_MINMAX: pairs (min, max), scale = max - min, < eps -> 1.  per_series = 0 reduces the column moments to one
 * pair in fixed-order fp64 (one workgroup: thread i adds columns i, i + 256, .. ascending, the 256 partials are added
 * ascending) and writes it to every column.
 *
 * ftn_table_affine: one pass over x [outer][S][inner] (series along the middle axis; element strides x_ostride,
 * x_sstride, and 1 along inner; the output likewise; out may be x):
 *   transform  out = ((FTN_TAB_CLIP ? (x < 0 ? 0 : x) : x) - loc[c]) / scale[c]
 *   inverse    (FTN_TAB_INVERSE) r = x * scale[c] + loc[c]; out = FTN_TAB_CLIP ? (r < 0 ? 0 : r) : r
 * c = s, or series[s] (int64 [S], clamped to 0 .. n_cols - 1 when read) with a series map.  fp32 with one rounding
 * per operation - a correctly rounded subtract and divide, a multiply and an add that are not contracted - so for
 * the same loc and scale bits the result is numpy's bit for bit.  16-byte lanes where x and out are 16-byte aligned,
 * the outer strides are multiples of 4 and either inner % 4 == 0 with series strides that are multiples of 4
 * (lane_axis 1) or inner == 1, S % 4 == 0 and both series strides 1 (lane_axis 2); 4-byte lanes otherwise; the same
 * bits either way.  S inner < 2^31 - 1024, S <= n_cols without a map.
 *
 * ftn_table_*_form: host-only; the launches dispatch through the same functions.  FtnTableForm: load_bytes 16 | 4;
 * col_tile (moments: 1024 | 256 columns a workgroup; spectrum: 64); block (moments: rows a block; spectrum: bins a
 * block; affine: elements a unit); chunk (spectrum: rows a staging chunk); resident (spectrum: 1 when the whole column
 * tile is one chunk, 0 when it is streamed); partials (moments: row blocks; spectrum: bin blocks); lane_axis (affine). */
#define FTN_TAB_CLIP 1
#define FTN_TAB_MASK 2
#define FTN_TAB_DIFF 4
#define FTN_TAB_INVERSE 8
#define FTN_TAB_ZSCORE 0
#define FTN_TAB_MINMAX 1
#define FTN_TAB_PARTIALS_MAX 32
#define FTN_TAB_SPEC_COLS 64
#define FTN_TAB_SPEC_BINS 128
#define FTN_TAB_SPEC_CHUNK 128
typedef struct FtnTableForm {
  int32_t load_bytes, col_tile, block, chunk, resident, partials, lane_axis, reserved;
} FtnTableForm;
typedef struct FtnTableMomentsArgs {
  const float* X; long long x_stride;
  const float* M; long long m_stride;
  long long T; int32_t N, flags;
  double* stats;
  void* workspace; size_t workspace_bytes;
} FtnTableMomentsArgs;
typedef struct FtnTableSpectrumArgs {
  const float* X; long long x_stride;
  const float* M; long long m_stride;
  const float* mean; const float* twiddle;
  long long T; int32_t N, reserved;
  int32_t* f_peak; float* peak; float* total; float* power_out;
  void* workspace; size_t workspace_bytes;
} FtnTableSpectrumArgs;
typedef struct FtnTableAffineArgs {
  const float* x; float* out;
  long long x_ostride, x_sstride, o_ostride, o_sstride, outer;
  int32_t S, inner, n_cols, flags;
  const float* loc; const float* scale; const long long* series;
} FtnTableAffineArgs;
size_t ftn_table_moments_bytes(long long T, int N);
int ftn_table_moments_form(const FtnTableMomentsArgs* args, FtnTableForm* form);
int ftn_table_moments(const FtnTableMomentsArgs* args, void* stream);
size_t ftn_table_twiddle_bytes(long long T);
int ftn_table_twiddle_init(void* table_dev, long long T, void* stream);
size_t ftn_table_spectrum_bytes(long long T, int N);
int ftn_table_spectrum_form(const FtnTableSpectrumArgs* args, FtnTableForm* form);
int ftn_table_spectrum(const FtnTableSpectrumArgs* args, void* stream);
int ftn_table_features(const double* stats_dev, const int32_t* f_peak_dev, const float* peak_dev,
                       const float* total_dev, long long T, int N, float* out_dev, void* stream);
int ftn_table_scaler(const double* stats_dev, int N, int method, int per_series, double eps, float* loc_dev,
                     float* scale_dev, float* pairs_dev, void* stream);
int ftn_table_affine_form(const FtnTableAffineArgs* args, FtnTableForm* form);
int ftn_table_affine(const FtnTableAffineArgs* args, void* stream);

/* ---- measurement ---------------------------------------------------------------- */
/* hipEvent brackets around the 6 stages (A pw-in, B conv, C fused pointwise chain,
 * D conv, E pw-out, F combine) of the following ftn_timesblock_forward calls - every
 * `enable`-th call (1 = every call, 0 = off; the events themselves cost ~3 us each on the
 * stream), up to 512 recorded calls; nothing synchronises until ftn_stage_times is called.
 * The first enabling call creates the events (host time): do it outside a timed region. */
int ftn_stage_timing(int enable);
/* sums, over the calls recorded since ftn_stage_timing(1), of each stage's elapsed
 * milliseconds; synchronises on the recorded events.  nstage must be 6. */
int ftn_stage_times(float* ms_sum_host, int nstage, int* ncalls_host);

/* Diagnostic: register (or clear with NULL) a device buffer of n_u64 64-bit words; thread 0 of
 * every following k_conv / k_mlp workgroup stores s_memtime at its phase boundaries in
 * words [8*wg .. 8*wg+7].  The last registered conv/mlp launch wins; not for production. */
int ftn_debug_stamps(void* buf_dev, size_t n_u64, int which /* 1: k_conv, 2: k_mlp */);

/* ---- diagnostics --------------------------------------------------------------- */
/* writes D = A(16x8, a[i][k]=i*8+k+1) * B(8x16, b[k][j]=(k+1)*100+j) via two
 * v_mfma_f32_16x16x4_f32 to out[16][16]: verifies the lane maps the kernels assume */
int ftn_selftest_mfma(float* out_dev, void* stream);
/* Diagnostic: out[i] = GELU(in[i]) exactly as the kernels evaluate nn.GELU() (erf form, :643). */
int ftn_selftest_gelu(const float* in_dev, float* out_dev, long long n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FLOWTIMES_H */
