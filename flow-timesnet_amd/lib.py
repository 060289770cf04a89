"""ctypes binding of ``csrc/libflowtimes_hip.so`` (C ABI: ``include/flowtimes.h``).

The library is loaded lazily and loudly: there is no CPU or PyTorch substitute
behind these calls.  ``load()`` raises ``FlowTimesLibraryError`` if the shared
object is missing or does not export every symbol the header declares.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path
from typing import Optional

FTN_KMAX = 16
FTN_MAXBR = 8
ABI_VERSION = 14

_HERE = Path(__file__).resolve().parent
LIB_PATH = _HERE / "csrc" / "libflowtimes_hip.so"


class FlowTimesLibraryError(RuntimeError):
    pass


FTN_XCHG_MAXWORLD = 16


class FtnExchange(C.Structure):
    """Mirror of ``struct FtnExchange`` (include/flowtimes.h): the peer-mapped exchange buffers of a batch-sharded run."""

    _fields_ = [("slots", C.c_void_p * FTN_XCHG_MAXWORLD), ("world", C.c_int32), ("rank", C.c_int32),
                ("F_cap", C.c_int32), ("seq", C.c_uint64), ("mode", C.c_int32)]


FTN_ROWX_CHUNK = 16384


class FtnRowExchange(C.Structure):
    """Mirror of ``struct FtnRowExchange`` (include/flowtimes.h): the peer-mapped row buffers of a series-sharded run
    (``kind`` 0 = reduce-scatter, 1 = all-gather)."""

    _fields_ = [("slots", C.c_void_p * FTN_XCHG_MAXWORLD), ("world", C.c_int32), ("rank", C.c_int32),
                ("rows_per_rank", C.c_int32), ("width", C.c_int32), ("kind", C.c_int32), ("reserved", C.c_int32)]


class FtnScorePart(C.Structure):
    """Mirror of ``struct FtnScorePart`` (include/flowtimes.h): what scoring leaves per column and per slot."""

    _fields_ = [("nll_sum", C.c_double), ("smape_sum", C.c_double), ("nll_cnt", C.c_int32), ("smape_cnt", C.c_int32)]


SCORE_PART_BYTES = C.sizeof(FtnScorePart)
FTN_QMAX = 8
FTN_NBG_PARTS_MAX = 1024
FTN_HEADFIT_COLSUM, FTN_HEADFIT_MFMA, FTN_HEADFIT_CHUNKS_MAX = 1, 2, 256
FTN_TIMEPROJ_BWD_MFMA, FTN_TIMEPROJ_BWD_CHUNKS_MAX, TIMEPROJ_BWD_CHUNK = 1, 256, 8
FTN_REFIT_MAX_TENSORS, FTN_REFIT_MAX_SKIP, FTN_REFIT_PARTS_MAX = 8, 8, 1024
FTN_REFIT_ONE, FTN_REFIT_GRID = 1, 2
FTN_REFIT_LIST_MAX = 4                 # records of one ftn_refit_update_list step
FTN_LATEFIT_MFMA, FTN_LATEFIT_CHUNKS_MAX, LATEFIT_CHUNK = 1, 256, 256
FTN_REFIT_ROWS_BAD = 4                 # ftn_refit_rows_gather's status word when a row index was outside the store


class FtnRefitArgs(C.Structure):
    """Mirror of ``struct FtnRefitArgs`` (include/flowtimes.h): the operands of one clip-and-AdamW call."""

    _fields_ = [("p", C.c_void_p * FTN_REFIT_MAX_TENSORS), ("g", C.c_void_p * FTN_REFIT_MAX_TENSORS),
                ("m", C.c_void_p * FTN_REFIT_MAX_TENSORS), ("v", C.c_void_p * FTN_REFIT_MAX_TENSORS),
                ("n", C.c_longlong * FTN_REFIT_MAX_TENSORS), ("n_tensors", C.c_int32), ("n_skip", C.c_int32),
                ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double), ("weight_decay", C.c_double),
                ("max_norm", C.c_double), ("lr", C.c_void_p), ("state", C.c_void_p),
                ("skip", C.c_void_p * FTN_REFIT_MAX_SKIP), ("range_mask", C.c_int32), ("log_cap", C.c_int32),
                ("loss", C.c_void_p), ("log", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
                ("force_form", C.c_int32), ("reserved", C.c_int32)]


FTN_EPOCH_MAX_TENSORS = 8
FTN_EPOCH_STOP, FTN_EPOCH_AFTER_STOP, FTN_EPOCH_SCORER_ERR = 16, 16, 32
FTN_EPOCH_COPY_VEC, FTN_EPOCH_COPY_MIXED = 1, 2


class FtnEpochState(C.Structure):
    """Mirror of ``struct FtnEpochState`` (include/flowtimes.h): what a validated refit carries from epoch to epoch."""

    _fields_ = [("best_nll", C.c_double), ("best_smape", C.c_double), ("plateau_best", C.c_double), ("lr", C.c_double),
                ("epoch", C.c_int32), ("best_epoch", C.c_int32), ("patience", C.c_int32), ("num_bad", C.c_int32),
                ("stop", C.c_int32), ("improved", C.c_int32), ("calls", C.c_int32), ("reserved", C.c_int32)]


class FtnEpochArgs(C.Structure):
    """Mirror of ``struct FtnEpochArgs`` (include/flowtimes.h): the operands of one ``ftn_refit_epoch_end``."""

    _fields_ = [("acc", C.c_void_p), ("n_slots", C.c_int32), ("max_epochs", C.c_int32), ("err", C.c_void_p),
                ("den_extra", C.c_void_p), ("count_seen", C.c_void_p), ("state", C.c_void_p), ("lr", C.c_void_p),
                ("log", C.c_void_p), ("factor", C.c_double), ("threshold", C.c_double), ("min_lr", C.c_double),
                ("plateau_patience", C.c_int32), ("patience_limit", C.c_int32),
                ("src", C.c_void_p * FTN_EPOCH_MAX_TENSORS), ("dst", C.c_void_p * FTN_EPOCH_MAX_TENSORS),
                ("n", C.c_longlong * FTN_EPOCH_MAX_TENSORS), ("n_tensors", C.c_int32), ("reserved", C.c_int32)]


FTN_NBQ_RANGE = 2
FTN_PATHS_MAX = 1024
FTN_PATH_SUM, FTN_PATH_MAX = 0, 1
FTN_PATH_LDS = 16
FTN_GROUP_CHUNK = 32
FTN_GROUP_NMAX, FTN_GROUP_GMAX, FTN_GROUP_CHUNKS_MAX = 8192, 2048, 2048
FTN_GROUP_TILE_BYTES, FTN_GROUP_TILE_ROWS = 32768, 64
FTN_GROUP_TILE_COLS = 64


class FtnDesc(C.Structure):
    """Mirror of ``struct FtnDesc`` (include/flowtimes.h)."""

    _fields_ = [
        ("n_sel", C.c_int32), ("n_groups", C.c_int32), ("total_px", C.c_int32), ("tiles_per_row", C.c_int32),
        ("sel_freq", C.c_int32 * FTN_KMAX), ("sel_period", C.c_int32 * FTN_KMAX), ("sel_group", C.c_int32 * FTN_KMAX),
        ("g_period", C.c_int32 * FTN_KMAX), ("g_pad", C.c_int32 * FTN_KMAX), ("g_cycles", C.c_int32 * FTN_KMAX),
        ("g_px_off", C.c_int32 * (FTN_KMAX + 1)),
        ("g_tw", C.c_int32 * FTN_KMAX), ("g_th", C.c_int32 * FTN_KMAX),
        ("g_ntx", C.c_int32 * FTN_KMAX), ("g_nty", C.c_int32 * FTN_KMAX),
        ("g_tile_off", C.c_int32 * (FTN_KMAX + 1)),
    ]


DESC_INTS = C.sizeof(FtnDesc) // 4


class FtnPlan(C.Structure):
    """Mirror of ``struct FtnPlan`` (include/flowtimes.h)."""

    _fields_ = [
        ("C", C.c_int32), ("CP", C.c_int32), ("F", C.c_int32), ("FP", C.c_int32),
        ("mode", C.c_int32), ("act", C.c_int32), ("nbr", C.c_int32), ("MP", C.c_int32),
        ("kh", C.c_int32 * FTN_MAXBR), ("kw", C.c_int32 * FTN_MAXBR),
        ("res1", C.c_int32), ("res2", C.c_int32),
        ("w_in1", C.c_int64), ("b_in1", C.c_int64),
        ("w_conv1", C.c_int64 * FTN_MAXBR), ("b_conv1", C.c_int64),
        ("w_out1", C.c_int64), ("b_out1", C.c_int64),
        ("w_res1", C.c_int64), ("b_res1", C.c_int64),
        ("w_in2", C.c_int64), ("b_in2", C.c_int64),
        ("w_conv2", C.c_int64 * FTN_MAXBR), ("b_conv2", C.c_int64),
        ("w_out2", C.c_int64), ("b_out2", C.c_int64),
        ("w_res2", C.c_int64), ("b_res2", C.c_int64),
        ("w_c2", C.c_int64), ("b_c2", C.c_int64),
        ("w_cfrag", C.c_int64), ("cfrag_per_chunk", C.c_int32), ("n_hchunks", C.c_int32),
        ("w_convbf1", C.c_int64 * FTN_MAXBR), ("w_convbf2", C.c_int64 * FTN_MAXBR),
        ("engine", C.c_int32), ("cfragbf_per_chunk", C.c_int32), ("w_cfragbf", C.c_int64),
        ("b_conv1s", C.c_int64), ("b_conv2s", C.c_int64), ("b_out1s", C.c_int64), ("b_res1s", C.c_int64),
        ("b_c2s", C.c_int64),
        ("sc_conv1", C.c_float * FTN_MAXBR), ("sc_conv2", C.c_float * FTN_MAXBR),
        ("sc_out1", C.c_float), ("sc_res1", C.c_float), ("sc_a2", C.c_float), ("sc_r2", C.c_float),
        ("w_out2fb", C.c_int64), ("b_out2s", C.c_int64), ("sc_out2", C.c_float), ("reserved0", C.c_int32),
        ("total_floats", C.c_int64),
    ]


class FtnForms(C.Structure):
    """Mirror of ``struct FtnForms`` (include/flowtimes.h): the kernel form each stage of a block call takes."""

    _fields_ = [(n, C.c_int32) for n in ("mode", "act", "nsplit", "xvec", "yvec", "stage_a_epi", "conv", "conv_n",
                                         "stage_c", "r_keeps_x", "r_summed", "stage_e", "half_round")] + [
        ("reserved", C.c_int32 * 3)]


class FtnContextParams(C.Structure):
    """Mirror of ``struct FtnContextParams`` (include/flowtimes.h): the parameters ``ftn_context_rows`` reads."""

    _fields_ = [(n, C.c_void_p) for n in ("w_s", "b_s", "sn_g", "sn_b", "emb", "cn_g", "cn_b", "w_c", "b_c", "w_p",
                                          "b_p", "ln_g", "ln_b", "w_l", "b_l", "gate")] + [
        (n, C.c_float) for n in ("sn_eps", "cn_eps", "ln_eps")] + [
        (n, C.c_int32) for n in ("F", "Ws", "Ed", "V", "R", "steps", "reserved")]


class FtnEmbedAddParams(C.Structure):
    """Mirror of ``struct FtnEmbedAddParams`` (include/flowtimes.h): the parameters ``ftn_embed_add`` reads."""

    _fields_ = [(n, C.c_void_p) for n in ("pos", "w_t", "b_t", "aux_g", "aux_b", "gate", "b_v", "basisc", "scale")] + [
        ("aux_eps", C.c_float), ("T", C.c_int32)]


FTN_CTX_MAX, FTN_CTX_RMAX, FTN_ADD_DMAX, FTN_ADD_TMAX = 256, 32, 512, 64
FTN_WIN_SERIES, FTN_WIN_WIDE = 0, 1
FTN_WIN_TILE_SERIES, FTN_WIN_TILE_STEPS = 64, 32


class FtnWindowArgs(C.Structure):
    """Mirror of ``struct FtnWindowArgs`` (include/flowtimes.h): the tables, the item range and the outputs of one
    ``ftn_window_batch`` call."""

    _fields_ = [("X", C.c_void_p), ("x_stride", C.c_longlong), ("M", C.c_void_p), ("m_stride", C.c_longlong),
                ("marks", C.c_void_p), ("marks_stride", C.c_longlong), ("statics", C.c_void_p), ("ids", C.c_void_p),
                ("starts", C.c_void_p), ("starts_host", C.c_void_p),
                ("T", C.c_longlong), ("item0", C.c_longlong), ("count", C.c_longlong)] + [
        (n, C.c_int32) for n in ("N", "L", "H", "F", "Fs", "W", "layout", "reserved")] + [
        (n, C.c_void_p) for n in ("x", "y", "mask", "x_mark", "y_mark", "static_out", "id_out")]


class FtnWindowGatherArgs(C.Structure):
    """Mirror of ``struct FtnWindowGatherArgs`` (include/flowtimes.h): an ``FtnWindowArgs`` (``item0`` is the part's
    first global item), the series-major tables, the item list and the epoch's generator words."""

    _fields_ = [("w", FtnWindowArgs), ("XT", C.c_void_p), ("xt_stride", C.c_longlong), ("MT", C.c_void_p),
                ("mt_stride", C.c_longlong), ("items", C.c_void_p), ("seed", C.c_ulonglong),
                ("noise_std", C.c_double), ("epoch", C.c_uint32), ("ts", C.c_int32)]


FTN_TAB_CLIP, FTN_TAB_MASK, FTN_TAB_DIFF, FTN_TAB_INVERSE = 1, 2, 4, 8
FTN_TAB_ZSCORE, FTN_TAB_MINMAX = 0, 1
FTN_TAB_PARTIALS_MAX, FTN_TAB_SPEC_COLS, FTN_TAB_SPEC_BINS, FTN_TAB_SPEC_CHUNK = 32, 64, 128, 128
FTN_TAB_T_MAX = 65536


class FtnTableForm(C.Structure):
    """Mirror of ``struct FtnTableForm`` (include/flowtimes.h): what a ``ftn_table_*_form`` query reports."""

    _fields_ = [(n, C.c_int32) for n in ("load_bytes", "col_tile", "block", "chunk", "resident", "partials",
                                         "lane_axis", "reserved")]


class FtnTableMomentsArgs(C.Structure):
    """Mirror of ``struct FtnTableMomentsArgs`` (include/flowtimes.h)."""

    _fields_ = [("X", C.c_void_p), ("x_stride", C.c_longlong), ("M", C.c_void_p), ("m_stride", C.c_longlong),
                ("T", C.c_longlong), ("N", C.c_int32), ("flags", C.c_int32), ("stats", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t)]


class FtnTableSpectrumArgs(C.Structure):
    """Mirror of ``struct FtnTableSpectrumArgs`` (include/flowtimes.h)."""

    _fields_ = [("X", C.c_void_p), ("x_stride", C.c_longlong), ("M", C.c_void_p), ("m_stride", C.c_longlong),
                ("mean", C.c_void_p), ("twiddle", C.c_void_p), ("T", C.c_longlong), ("N", C.c_int32),
                ("reserved", C.c_int32), ("f_peak", C.c_void_p), ("peak", C.c_void_p), ("total", C.c_void_p),
                ("power_out", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t)]


class FtnTableAffineArgs(C.Structure):
    """Mirror of ``struct FtnTableAffineArgs`` (include/flowtimes.h)."""

    _fields_ = [("x", C.c_void_p), ("out", C.c_void_p)] + [
        (n, C.c_longlong) for n in ("x_ostride", "x_sstride", "o_ostride", "o_sstride", "outer")] + [
        (n, C.c_int32) for n in ("S", "inner", "n_cols", "flags")] + [
        ("loc", C.c_void_p), ("scale", C.c_void_p), ("series", C.c_void_p)]


class FtnInceptionBlockWeights(C.Structure):
    """Mirror of ``struct FtnInceptionBlockWeights`` (include/flowtimes.h): raw host pointers to the reference
    ``state_dict`` tensors of one InceptionBlock."""

    _fields_ = [
        ("branch_w", (C.c_void_p * 3) * FTN_MAXBR), ("branch_b", (C.c_void_p * 3) * FTN_MAXBR),
        ("proj_w", C.c_void_p), ("proj_b", C.c_void_p), ("res_w", C.c_void_p), ("res_b", C.c_void_p),
    ]


_P = C.c_void_p
_SIGNATURES = {
    # name: (restype, argtypes)            -- one entry per declaration in flowtimes.h
    "ftn_abi_version": (C.c_int, []),
    "ftn_last_error": (C.c_char_p, []),
    "ftn_inception_pack_floats": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                              C.c_double, C.c_int]),
    "ftn_inception_pack_weights": (C.c_int, [C.POINTER(FtnInceptionBlockWeights), C.POINTER(FtnInceptionBlockWeights),
                                             C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                             C.c_double, C.c_int, C.c_int, _P, C.c_size_t, C.POINTER(FtnPlan)]),
    "ftn_dft_table_bytes": (C.c_size_t, [C.c_int]),
    "ftn_dft_table_init": (C.c_int, [_P, C.c_int, _P]),
    "ftn_period_spectrum_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "ftn_period_spectrum": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, C.POINTER(FtnExchange), _P]),
    "ftn_exchange_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "ftn_exchange_error": (C.c_int, [C.POINTER(FtnExchange), _P]),
    "ftn_exchange_counter_offset": (C.c_size_t, [C.c_int, C.c_int]),
    "ftn_exchange_calls": (C.c_int64, [C.POINTER(FtnExchange), _P]),
    "ftn_exchange_alloc": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_void_p), _P]),
    "ftn_exchange_open": (C.c_int, [_P, C.POINTER(C.c_void_p)]),
    "ftn_exchange_close": (C.c_int, [_P]),
    "ftn_exchange_free": (C.c_int, [_P]),
    "ftn_rowx_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "ftn_rowx_alloc": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p), _P]),
    "ftn_rowx_open": (C.c_int, [_P, C.POINTER(C.c_void_p)]),
    "ftn_rowx_close": (C.c_int, [_P]),
    "ftn_rowx_free": (C.c_int, [_P]),
    "ftn_rowx_error": (C.c_int, [C.POINTER(FtnRowExchange), _P]),
    "ftn_rowx_calls": (C.c_int64, [C.POINTER(FtnRowExchange), _P]),
    "ftn_rowx_push": (C.c_int, [_P, C.POINTER(FtnRowExchange), _P]),
    "ftn_rowx_reduce": (C.c_int, [C.POINTER(FtnRowExchange), C.c_int, C.c_int, _P, C.c_longlong, _P, _P, C.c_float,
                                  _P, _P]),
    "ftn_rowx_gather": (C.c_int, [C.POINTER(FtnRowExchange), _P, _P]),
    "ftn_period_finalize": (C.c_int, [_P, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_int, C.c_double, _P, _P, _P, _P, C.POINTER(FtnExchange)]),
    "ftn_desc_from_periods": (C.c_int, [C.POINTER(C.c_int64), C.c_int, C.c_int, C.c_int, C.c_int,
                                        C.POINTER(FtnDesc)]),
    "ftn_selector_px_bound": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "ftn_timesblock_workspace_bytes": (C.c_size_t, [C.POINTER(FtnPlan), C.c_int, C.c_int, C.c_int, C.c_int]),
    "ftn_timesblock_forward": (C.c_int, [_P, _P, C.c_int, C.c_int, C.POINTER(FtnPlan), _P, _P, _P, C.c_int, C.c_int,
                                         C.c_int, C.c_int, _P, C.c_size_t, _P, _P]),
    "ftn_timesblock_forward_norm": (C.c_int, [_P, _P, C.c_int, C.c_int, C.POINTER(FtnPlan), _P, _P, _P, C.c_int,
                                              C.c_int, C.c_int, _P, _P, C.c_float, _P, C.c_size_t, _P, _P]),
    # row passes: the two forwards above with rows_per_pass appended, and the host-only pass size for a workspace cap
    "ftn_timesblock_forward_rows": (C.c_int, [_P, _P, C.c_int, C.c_int, C.POINTER(FtnPlan), _P, _P, _P, C.c_int,
                                              C.c_int, C.c_int, C.c_int, _P, C.c_size_t, _P, _P, C.c_int]),
    "ftn_timesblock_forward_norm_rows": (C.c_int, [_P, _P, C.c_int, C.c_int, C.POINTER(FtnPlan), _P, _P, _P, C.c_int,
                                                   C.c_int, C.c_int, _P, _P, C.c_float, _P, C.c_size_t, _P, _P,
                                                   C.c_int]),
    "ftn_timesblock_rows_per_pass": (C.c_int, [C.POINTER(FtnPlan), C.c_int, C.c_int, C.c_int, C.c_size_t]),
    "ftn_period_finalize_stage_a": (C.c_int, [_P, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                              C.c_int, C.c_int, C.c_double, _P, _P, _P, _P, C.POINTER(FtnPlan), _P,
                                              C.c_int, C.c_int, _P, C.c_size_t, _P, _P, C.POINTER(FtnExchange)]),
    "ftn_residual_layernorm": (C.c_int, [_P, _P, _P, C.c_longlong, C.c_int, _P, _P, C.c_float, _P]),
    "ftn_timesblock_forms": (C.c_int, [C.POINTER(FtnPlan), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(FtnForms)]),
    "ftn_period_spectrum_form": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "ftn_head_forward": (C.c_int, [_P, C.c_longlong, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, C.c_longlong,
                                   C.c_int, _P, C.c_longlong, _P, C.c_float, _P, _P, _P, _P]),
    "ftn_embed_forward": (C.c_int, [_P, C.c_longlong, C.c_int, C.c_int, C.c_int, _P, C.c_int, _P, C.c_longlong,
                                    _P, _P, C.c_float, _P, _P]),
    "ftn_embed_rows_strided": (C.c_int, [_P, C.c_longlong, C.c_int, C.c_int, C.c_int, _P, C.c_int, _P, C.c_longlong,
                                         _P]),
    "ftn_embed_ring": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_longlong, _P, _P, C.c_float, _P,
                                 _P]),
    "ftn_embed_form": (C.c_int, [C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int]),
    "ftn_head_form": (C.c_int, [C.c_int, C.c_int, C.c_longlong, C.c_longlong, C.c_int]),
    "ftn_timeproj_forward": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, _P, _P]),
    "ftn_timeproj_form": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int]),
    # 128 < d_model <= 512: the signatures of the narrow entry points above
    "ftn_embed_wide_forward": (C.c_int, [_P, C.c_longlong, C.c_int, C.c_int, C.c_int, _P, C.c_int, _P, C.c_longlong,
                                         _P, _P, C.c_float, _P, _P]),
    "ftn_embed_wide_rows_strided": (C.c_int, [_P, C.c_longlong, C.c_int, C.c_int, C.c_int, _P, C.c_int, _P,
                                              C.c_longlong, _P]),
    "ftn_embed_wide_ring": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_longlong, _P, _P, C.c_float, _P,
                                      _P]),
    "ftn_head_wide_forward": (C.c_int, [_P, C.c_longlong, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, C.c_longlong,
                                        C.c_int, _P, C.c_longlong, _P, C.c_float, _P, _P, _P, _P]),
    "ftn_timeproj_wide_forward": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, _P, _P]),
    "ftn_embed_wide_form": (C.c_int, [C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int]),
    "ftn_head_wide_form": (C.c_int, [C.c_int, C.c_int, C.c_longlong, C.c_longlong, C.c_int]),
    "ftn_timeproj_wide_form": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int]),
    # embed_norm_mode "rms": the signatures of the LayerNorm entry points, gamma and beta required
    "ftn_embed_forward_rms": (C.c_int, [_P, C.c_longlong, C.c_int, C.c_int, C.c_int, _P, C.c_int, _P, C.c_longlong,
                                        _P, _P, C.c_float, _P, _P]),
    "ftn_embed_ring_rms": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_longlong, _P, _P, C.c_float, _P,
                                     _P]),
    "ftn_embed_wide_forward_rms": (C.c_int, [_P, C.c_longlong, C.c_int, C.c_int, C.c_int, _P, C.c_int, _P,
                                             C.c_longlong, _P, _P, C.c_float, _P, _P]),
    "ftn_embed_wide_ring_rms": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_longlong, _P, _P, C.c_float,
                                          _P, _P]),
    "ftn_score_form": (C.c_int, [C.c_int, C.c_int, C.c_longlong, C.c_longlong, C.c_longlong, C.c_int]),
    "ftn_score_columns": (C.c_int, [_P, C.c_longlong, _P, C.c_longlong, _P, C.c_longlong, _P, C.c_int, C.c_float,
                                    C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    "ftn_score_fold": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, C.c_int, _P, _P]),
    # head refit (csrc/headfit.hip)
    "ftn_nb_nll_grad_form": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_longlong, C.c_longlong, C.c_int]),
    "ftn_nb_nll_grad_workspace": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "ftn_nb_nll_grad": (C.c_int, [_P, C.c_longlong, _P, C.c_longlong, _P, C.c_longlong, _P, C.c_int, C.c_float,
                                  C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, C.c_size_t, C.c_int, _P]),
    "ftn_head_backward_form": (C.c_int, [C.c_longlong, C.c_int, C.c_int, C.c_int]),
    "ftn_head_backward_workspace": (C.c_size_t, [C.c_longlong, C.c_int, C.c_int]),
    "ftn_head_fit_forward": (C.c_int, [_P, C.c_longlong, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, C.c_longlong,
                                       C.c_int, _P, C.c_longlong, _P, C.c_float, _P, _P, _P, _P, _P, _P]),
    "ftn_head_backward": (C.c_int, [_P, C.c_longlong, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                    _P, _P, C.c_size_t, _P]),
    # time projection backward (csrc/timeproj_bwd.hip)
    "ftn_timeproj_backward_form": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "ftn_timeproj_backward_workspace": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "ftn_timeproj_backward": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, C.c_size_t, _P]),
    # cached refit: the row-mapped time projection (csrc/timeproj.hip, timeproj_bwd.hip), the batch gather
    # (csrc/refit_rows.hip)
    "ftn_timeproj_forward_rows": (C.c_int, [_P, C.c_longlong, _P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, _P, _P]),
    "ftn_timeproj_wide_forward_rows": (C.c_int, [_P, C.c_longlong, _P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, _P,
                                                 _P]),
    "ftn_timeproj_backward_rows": (C.c_int, [_P, C.c_longlong, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P,
                                             C.c_size_t, _P]),
    "ftn_refit_rows_gather": (C.c_int, [_P, C.c_int, C.c_longlong, _P, C.c_int, _P, _P, _P, C.c_int, _P, _P, _P, _P, _P,
                                        _P, _P]),
    # refit step: clip and AdamW (csrc/refit.hip)
    "ftn_refit_update_form": (C.c_int, [C.c_int, C.POINTER(C.c_longlong), C.POINTER(C.c_int)]),
    "ftn_refit_update_workspace": (C.c_size_t, [C.c_int, C.POINTER(C.c_longlong)]),
    "ftn_refit_update": (C.c_int, [C.POINTER(FtnRefitArgs), _P]),
    "ftn_refit_update_list_workspace": (C.c_size_t, [C.c_int, C.POINTER(C.c_int),
                                                     C.POINTER(C.POINTER(C.c_longlong))]),
    "ftn_refit_update_list": (C.c_int, [C.POINTER(FtnRefitArgs), C.c_int, _P, C.c_size_t, _P]),
    "ftn_late_backward_form": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "ftn_late_backward_workspace": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "ftn_late_fit_forward": (C.c_int, [_P, C.c_longlong, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, C.c_float, _P,
                                       _P, _P, _P, _P]),
    "ftn_late_backward": (C.c_int, [_P, C.c_int, _P, C.c_longlong, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P,
                                    C.c_float, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_size_t, _P]),
    # validated refit: the end of an epoch (csrc/refit_epoch.hip)
    "ftn_refit_epoch_form": (C.c_int, [C.c_int, C.POINTER(C.c_longlong), C.POINTER(C.c_int)]),
    "ftn_refit_epoch_end": (C.c_int, [C.POINTER(FtnEpochArgs), _P]),
    "ftn_refit_epoch_restore": (C.c_int, [_P, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                          C.POINTER(C.c_longlong), _P]),
    "ftn_nbq_form": (C.c_int, [C.c_int, C.c_longlong, C.c_longlong, C.c_longlong, C.c_int]),
    "ftn_nb_cdf": (C.c_int, [_P, C.c_longlong, _P, C.c_longlong, _P, C.c_longlong, C.c_int, C.c_int, C.c_int,
                             C.c_float, _P, _P, _P, _P]),
    "ftn_nb_quantiles": (C.c_int, [_P, C.c_longlong, _P, C.c_longlong, C.c_int, C.c_int, C.c_int,
                                   C.POINTER(C.c_double), C.c_int, C.c_float, _P, _P, _P]),
    "ftn_nb_sample_form": (C.c_int, [C.c_int, C.c_longlong, C.c_longlong, C.c_int]),
    "ftn_nb_sample": (C.c_int, [_P, C.c_longlong, _P, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_ulonglong,
                                _P, C.c_uint, C.c_float, _P, _P, _P, _P]),
    "ftn_path_summary_form": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_longlong, C.c_longlong, C.c_int]),
    "ftn_path_summary": (C.c_int, [_P, C.c_longlong, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                   C.c_int, _P, C.c_longlong, C.POINTER(C.c_int), C.c_int, _P, _P, _P, _P, _P]),
    "ftn_group_sum_form": (C.c_int, [C.c_int, C.c_longlong, C.c_int, C.c_int]),
    "ftn_group_sum": (C.c_int, [_P, C.c_longlong, C.c_int, C.c_longlong, _P, _P, _P, C.c_int, C.c_int, _P, _P]),
    "ftn_group_sum_rows_form": (C.c_int, [C.c_longlong, C.c_longlong, C.c_longlong, C.c_int, C.c_int]),
    "ftn_group_sum_rows": (C.c_int, [_P, C.c_longlong, C.c_int, C.c_longlong, C.c_longlong, C.c_longlong, _P, _P, _P,
                                     C.c_int, C.c_int, _P, _P]),
    # context front end (csrc/context.hip)
    "ftn_context_rows_form": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "ftn_context_rows": (C.c_int, [C.POINTER(FtnContextParams), _P, C.c_longlong, _P, C.c_longlong, C.c_int, C.c_int,
                                   _P, _P, _P, _P, _P]),
    "ftn_context_through_weight": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_longlong, C.c_int, _P, _P,
                                             _P]),
    "ftn_embed_add_form": (C.c_int, [C.c_int, C.c_longlong, C.c_longlong, C.c_int]),
    "ftn_embed_add": (C.c_int, [C.POINTER(FtnEmbedAddParams), _P, C.c_longlong, _P, C.c_longlong, C.c_int, _P,
                                C.c_longlong, C.c_int, C.c_int, C.c_int, _P, _P]),
    # device windows (csrc/windows.hip)
    "ftn_window_batch_form": (C.c_int, [C.POINTER(FtnWindowArgs)]),
    "ftn_window_batch": (C.c_int, [C.POINTER(FtnWindowArgs), _P]),
    # training windows (csrc/windows_gather.hip)
    "ftn_epoch_keys": (C.c_int, [C.c_longlong, C.c_ulonglong, C.c_uint, _P, _P]),
    "ftn_window_gather": (C.c_int, [C.POINTER(FtnWindowGatherArgs), _P]),
    # table preparation (csrc/table.hip)
    "ftn_table_moments_bytes": (C.c_size_t, [C.c_longlong, C.c_int]),
    "ftn_table_moments_form": (C.c_int, [C.POINTER(FtnTableMomentsArgs), C.POINTER(FtnTableForm)]),
    "ftn_table_moments": (C.c_int, [C.POINTER(FtnTableMomentsArgs), _P]),
    "ftn_table_twiddle_bytes": (C.c_size_t, [C.c_longlong]),
    "ftn_table_twiddle_init": (C.c_int, [_P, C.c_longlong, _P]),
    "ftn_table_spectrum_bytes": (C.c_size_t, [C.c_longlong, C.c_int]),
    "ftn_table_spectrum_form": (C.c_int, [C.POINTER(FtnTableSpectrumArgs), C.POINTER(FtnTableForm)]),
    "ftn_table_spectrum": (C.c_int, [C.POINTER(FtnTableSpectrumArgs), _P]),
    "ftn_table_features": (C.c_int, [_P, _P, _P, _P, C.c_longlong, C.c_int, _P, _P]),
    "ftn_table_scaler": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_double, _P, _P, _P, _P]),
    "ftn_table_affine_form": (C.c_int, [C.POINTER(FtnTableAffineArgs), C.POINTER(FtnTableForm)]),
    "ftn_table_affine": (C.c_int, [C.POINTER(FtnTableAffineArgs), _P]),
    "ftn_lrtc_basis_floats": (C.c_size_t, [C.c_int, C.c_int]),
    "ftn_lrtc_basis": (C.c_int, [_P, C.c_int, C.c_int, _P]),
    "ftn_lrtc_forward": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "ftn_lrtc_form": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "ftn_stage_timing": (C.c_int, [C.c_int]),
    "ftn_stage_times": (C.c_int, [C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_int)]),
    "ftn_debug_stamps": (C.c_int, [_P, C.c_size_t, C.c_int]),
    "ftn_selftest_mfma": (C.c_int, [_P, _P]),
    "ftn_selftest_gelu": (C.c_int, [_P, _P, C.c_longlong, _P]),
}
EXPORTS = tuple(_SIGNATURES)

_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """Load the shared library (once) and bind every exported symbol."""
    global _lib
    if _lib is not None:
        return _lib
    path = Path(os.environ.get("FLOWTIMES_LIB", LIB_PATH))
    build_log = ""
    if "FLOWTIMES_LIB" not in os.environ:
        # In-tree build on every first use (hipcc cross-compiles gfx950 without a GPU): `make` is a no-op when
        # the library is newer than its sources and rebuilds it when it is not, so a stale .so (it is git-ignored
        # but travels with the tree) can never be what the tests validate.  A failed build is an error with the
        # compiler's output attached, never a fallback.
        import shutil
        import subprocess

        hipcc = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if Path("/opt/rocm/bin/hipcc").exists() else None)
        csrc = _HERE / "csrc"

        def current() -> bool:
            """The library exists and is newer than every source it is built from."""
            if not path.exists():
                return False
            srcs = [*csrc.glob("*.hip"), *csrc.glob("*.h"), csrc / "Makefile", _HERE.parent / "include" / "flowtimes.h"]
            return all(not f.exists() or f.stat().st_mtime <= path.stat().st_mtime for f in srcs)

        if shutil.which("make") and hipcc and not (current() and not os.access(csrc, os.W_OK)):
            import fcntl

            # one builder at a time: the ranks of a multi-GPU launch all arrive here together
            try:
                lock = open(csrc / ".build.lock", "w")
            except OSError as exc:                              # read-only tree (an installed copy)
                if not current():
                    raise FlowTimesLibraryError(f"{csrc} is not writable and {path} is missing or older than its "
                                                f"sources: {exc}") from exc
                lock = None
            if lock is not None:
                with lock:
                    fcntl.flock(lock, fcntl.LOCK_EX)
                    try:
                        proc = subprocess.run(["make", "-C", str(csrc), "-j4"], check=False,
                                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
                        if proc.returncode != 0:
                            build_log = proc.stdout[-4000:]
                    finally:
                        fcntl.flock(lock, fcntl.LOCK_UN)
            if build_log:
                # a broken toolchain beside a library that is provably current (newer than every source) is not a
                # stale-library risk: use it and say so; anything else stays an error
                if not current():
                    raise FlowTimesLibraryError(f"building {path} failed; there is no fallback path:\n{build_log}")
                import warnings

                warnings.warn(f"`make` failed but {path.name} is newer than all of its sources - using it.\n{build_log[-500:]}",
                              RuntimeWarning, stacklevel=2)
    # torch first: its bundled HIP runtime carries the soname the library links against, so the library binds to
    # that runtime.  Loaded before torch, the library would pull in a second HIP runtime from the ROCm install, and
    # the device pointers and streams torch hands over belong to the first one.
    import torch  # noqa: F401

    if not path.exists():
        raise FlowTimesLibraryError(
            f"{path} not found: build it with `make -C {_HERE / 'csrc'}` "
            "(or `python -c 'import __graft_entry__ as g; g.build()'`); there is no fallback path"
        )
    try:
        lib = C.CDLL(str(path))
    except OSError as exc:  # missing ROCm runtime etc.
        raise FlowTimesLibraryError(f"cannot load {path}: {exc}") from exc
    for name, (res, args) in _SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as exc:
            raise FlowTimesLibraryError(f"{path} does not export {name}") from exc
        fn.restype = res
        fn.argtypes = args
    if lib.ftn_abi_version() != ABI_VERSION:
        raise FlowTimesLibraryError(f"ABI version {lib.ftn_abi_version()} != {ABI_VERSION}")
    _lib = lib
    return lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().ftn_last_error().decode("utf-8", "replace")
        kind = ValueError if rc < 0 else RuntimeError
        raise kind(f"{what} failed (rc={rc}): {msg}")


def desc_from_periods(periods, L: int, min_period: int, max_period: int) -> FtnDesc:
    """Host-side PeriodGrouper (default flags) + conv tiling, via the C helper."""
    lib = load()
    K = len(periods)
    arr = (C.c_int64 * max(K, 1))(*[int(p) for p in periods])
    d = FtnDesc()
    check(lib.ftn_desc_from_periods(arr, K, int(L), int(min_period), int(max_period), C.byref(d)),
          "ftn_desc_from_periods")
    return d
