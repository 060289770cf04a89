"""Per-device HIP runtime state for the TimesBlock path: DFT twiddle tables,
LRTC bases, and the thin call wrappers that pass ``tensor.data_ptr()`` / the
current HIP stream into the C ABI.  Workspaces are allocated per call from
torch's caching allocator (stream- and graph-pool-safe; free after warm-up).

PyTorch is plumbing here (device memory + streams); every computation happens
in ``libflowtimes_hip.so``.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Dict, Tuple

import torch

from . import lib as _lib
from .lib import DESC_INTS, FTN_KMAX, FtnDesc, FtnPlan, check


def _stream(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _ptr(t: torch.Tensor) -> int:
    return t.data_ptr()


def _ptr_or_null(t):
    return None if t is None else t.data_ptr()


def _form(name: str, *args) -> int:
    """The form word of a host-only ``ftn_*_form`` function for integer ``args``; its error through ``check``."""
    f = getattr(_lib.load(), name)(*(int(a) for a in args))
    if f < 0:
        check(f, name)
    return f


def _batch_stride(t, B: int) -> int:
    """Elements between the batch rows of an optional contiguous ``[1|B, R, C]`` operand: 0 when one ``[R, C]`` block
    serves every row of the batch (or there is no operand)."""
    return t.shape[-2] * t.shape[-1] if t is not None and t.dim() == 3 and t.shape[0] == B and B > 1 else 0


def _norm_args(norm):
    """``(gamma pointer, beta pointer, eps)`` of an optional LayerNorm epilogue ``norm = (gamma, beta, eps)``."""
    g, b, eps = norm if norm is not None else (None, None, 0.0)
    return _ptr_or_null(g), _ptr_or_null(b), float(eps)


def _embed_norm(norm):
    """The norm epilogue of ``embed_forward`` / ``embed_ring``: ``(entry suffix, (gamma, beta, eps) or None)`` of
    ``norm`` = None, ``(gamma, beta, eps)`` (LayerNorm) or ``(gamma, beta, eps, "rms")`` (the ``_rms`` entries)."""
    if norm is None or len(norm) == 3:
        return "", norm
    if len(norm) != 4 or norm[3] != "rms":
        raise ValueError(f"norm must be (gamma, beta, eps) or (gamma, beta, eps, 'rms'), got {len(norm)} elements"
                         + (f" with kind {norm[3]!r}" if len(norm) == 4 else ""))
    if norm[0] is None or norm[1] is None:
        raise ValueError("the RMS norm needs gamma and beta")
    return "_rms", tuple(norm[:3])


def _workspace_bytes(lib, plan: FtnPlan, B: int, L: int, max_groups: int, px_bound: int) -> int:
    need = lib.ftn_timesblock_workspace_bytes(C.byref(plan), B, L, max_groups, px_bound)
    if need == 0:
        raise ValueError(f"ftn_timesblock_workspace_bytes rejected the shape (B={B}, L={L})")
    return need


def _workspace(device, need: int) -> torch.Tensor:
    """One TimesBlock workspace of ``_workspace_bytes`` per call, from the caching allocator: ordered on the calling
    stream, private to a graph capture's pool, never shared between calls in flight (a process-wide buffer would be)."""
    return torch.empty(need, dtype=torch.uint8, device=device)


class DeviceState:
    """Caches that live as long as the process, one instance per CUDA device."""

    def __init__(self, device: torch.device) -> None:
        self.device = device
        self.tables: Dict[int, torch.Tensor] = {}
        self.bases: Dict[Tuple[int, int], torch.Tensor] = {}
        self.twiddles: Dict[int, torch.Tensor] = {}             # table spectrum: 8 T bytes per history length T

    def dft_table(self, L: int) -> torch.Tensor:
        t = self.tables.get(L)
        if t is None:
            lib = _lib.load()
            nbytes = lib.ftn_dft_table_bytes(L)
            t = torch.empty(nbytes // 4, dtype=torch.float32, device=self.device)
            check(lib.ftn_dft_table_init(_ptr(t), L, _stream(self.device)), "ftn_dft_table_init")
            self.tables[L] = t
        return t

    def table_twiddles(self, T: int) -> torch.Tensor:
        """The ``T`` twiddles of ``ftn_table_spectrum`` (``ftn_table_twiddle_init``), cached per ``T``
        (the 64 most recently built)."""
        key = int(T)
        t = self.twiddles.get(key)
        if t is None:
            lib = _lib.load()
            nbytes = lib.ftn_table_twiddle_bytes(key)
            if nbytes == 0:
                raise ValueError(f"table spectrum: T={T} is outside 1..{_lib.FTN_TAB_T_MAX}")
            if len(self.twiddles) >= 64:                        # a pipeline whose history grows by the day: keep it bounded
                self.twiddles.pop(next(iter(self.twiddles)))
            t = torch.empty(nbytes // 4, dtype=torch.float32, device=self.device)
            check(lib.ftn_table_twiddle_init(_ptr(t), key, _stream(self.device)), "ftn_table_twiddle_init")
            self.twiddles[key] = t
        return t

    def lrtc_basis(self, L: int, R: int) -> torch.Tensor:
        key = (L, R)
        t = self.bases.get(key)
        if t is None:
            lib = _lib.load()
            t = torch.empty(lib.ftn_lrtc_basis_floats(L, R), dtype=torch.float32, device=self.device)
            check(lib.ftn_lrtc_basis(_ptr(t), L, R, _stream(self.device)), "ftn_lrtc_basis")
            self.bases[key] = t
        return t


_states: Dict[int, DeviceState] = {}


def state(device: torch.device) -> DeviceState:
    idx = device.index if device.index is not None else torch.cuda.current_device()
    st = _states.get(idx)
    if st is None:
        st = DeviceState(torch.device("cuda", idx))
        _states[idx] = st
    return st


# ------------------------------------------------------------------ selector
class Selection:
    """Device-resident result of the period selector for one block call."""

    def __init__(self, desc: torch.Tensor, amps: torch.Tensor, weights: torch.Tensor, max_groups: int,
                 px_bound: int = 0) -> None:
        self.desc = desc          # int32 [DESC_INTS]
        self.amps = amps          # [B, FTN_KMAX]
        self.weights = weights    # [B, FTN_KMAX]
        self.max_groups = max_groups     # >= desc.n_groups
        self.px_bound = px_bound         # >= desc.total_px (0: generic worst case)
        self.stage_a = None              # StageA of the consuming block when its stage A is done (finalize .. forward)
        self._host = None

    def host(self) -> FtnDesc:
        """Copy the descriptor to the host (synchronises the stream)."""
        if self._host is None:
            raw = self.desc.cpu().numpy().tobytes()
            self._host = FtnDesc.from_buffer_copy(raw)
        return self._host


def spectrum(x: torch.Tensor, xch=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """S1+S2 on the device: channel-median amplitude [B,F] and its fp64 batch sum [F].  ``xch`` (a ``ctypes.byref`` of
    an ``FtnExchange``): the sums are also stored into every rank's exchange buffer (``dist.IpcExchange``)."""
    lib = _lib.load()
    B, L, Cc = x.shape
    st = state(x.device)
    Fb = L // 2 + 1
    med = torch.empty(B, Fb, dtype=torch.float32, device=x.device)
    psum = torch.empty(Fb, dtype=torch.float64, device=x.device)
    nscr = int(lib.ftn_period_spectrum_scratch_bytes(B, L, Cc))      # > 0: the channel-tiled form of d_model > 64
    scratch = torch.empty(nscr, dtype=torch.uint8, device=x.device) if nscr else None
    check(lib.ftn_period_spectrum(_ptr(x), B, L, Cc, _ptr(st.dft_table(L)), _ptr(med), _ptr(psum),
                                  _stream(x.device), xch, _ptr_or_null(scratch)), "ftn_period_spectrum")
    return med, psum


ACT_DTYPE = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}


def _selector_bounds(lib, L: int, k: int, pmax: int, min_thr: int) -> Tuple[int, int]:
    mg = C.c_int(0)
    pxb = lib.ftn_selector_px_bound(L, int(k), int(pmax), int(min_thr), C.byref(mg))
    if pxb < 0:
        check(pxb, "ftn_selector_px_bound")
    return max(1, int(mg.value)), int(pxb)


def new_range_flag(device: torch.device) -> torch.Tensor:
    """One int32 the f16x2 kernels set when a value leaves the fp16 range (``include/flowtimes.h``, ABI 9).  By default
    it lives in pinned host memory, which the device writes directly (zero-copy): the host can then read it at any time
    without a copy or a synchronisation once the call's completion event has fired.  ``FTN_RANGE_FLAG=device`` keeps it
    in device memory (reading it then synchronises)."""
    if os.getenv("FTN_RANGE_FLAG", "host") == "device":
        return torch.zeros(1, dtype=torch.int32, device=device)
    return torch.zeros(1, dtype=torch.int32).pin_memory()


def fuse_stage_a(plan) -> bool:
    """Stage A can ride with the selector's finalize launch (bottleneck blocks; FTN_FUSE_STAGE_A=0 disables)."""
    return plan.mode == 0 and os.getenv("FTN_FUSE_STAGE_A", "1") != "0"


class StageA:
    """The block call that will consume a selection: its input ``x`` (fp32, contiguous), ``plan``, ``wblob`` and
    optional ``range_flag``.  Stage A (a = W_in1 x + b) needs nothing of the selection, so ``finalize`` runs it in
    the selector's launch, or ``stage_a_only`` ahead of it: ``ws`` is then the block's workspace, which holds it."""

    def __init__(self, x: torch.Tensor, plan: FtnPlan, wblob: torch.Tensor, range_flag: Optional[torch.Tensor] = None,
                 ws: Optional[torch.Tensor] = None) -> None:
        self.x, self.plan, self.wblob, self.range_flag, self.ws = x, plan, wblob, range_flag, ws

    @staticmethod
    def checked(call) -> Optional["StageA"]:
        if call is not None and not isinstance(call, StageA):
            raise TypeError(f"stage_a must be a runtime.StageA record, not {type(call).__name__}")
        return call


def stage_a_only(call: StageA, k: int, pmax: int, min_thr: int) -> None:
    """Stage A of ``call`` into a fresh workspace ``call.ws``, without the selection (``ftn_period_finalize_stage_a``
    with ``psum = NULL``): a batch-sharded run launches it between issuing the exchange of the partial sums and
    waiting for it.  ``finalize(..., stage_a=call)`` completes it."""
    lib = _lib.load()
    B, L, _ = call.x.shape
    dev = call.x.device
    mg, pxb = _selector_bounds(lib, L, k, pmax, min_thr)
    call.ws = _workspace(dev, _workspace_bytes(lib, call.plan, B, L, mg, pxb))
    check(lib.ftn_period_finalize_stage_a(None, 0, 0, None, B, L, int(k), int(pmax), int(min_thr), 0, 0, 0.0,
                                          None, None, None, _ptr(call.x), C.byref(call.plan), _ptr(call.wblob), mg, pxb,
                                          _ptr(call.ws), call.ws.numel(), _stream(dev), _ptr_or_null(call.range_flag),
                                          None), "ftn_period_finalize_stage_a")


def finalize(psum: torch.Tensor, b_total: int, med: torch.Tensor, L: int, k: int, pmax: int,
             min_thr: int, act_dtype: int = 0, max_unique: int = 0, log_base: float = 0.0,
             stage_a: Optional[StageA] = None, xch=None) -> Selection:
    """S3-S5 on the device.  ``psum`` is [F] or [nparts, F] (multi-GPU partial sums); ``act_dtype`` 1 / 2
    applies the reference's bf16 / fp16 roundings of scores, amplitudes and weights.

    ``stage_a``: the block call that consumes this selection is known, so its stage A rides in the same launch
    (``ftn_period_finalize_stage_a``) when ``fuse_stage_a`` allows; after ``stage_a_only`` only S3-S5 and the
    descriptor copy remain.  Either way the returned Selection carries the record, whose ``ws`` is the block's
    workspace, and ``timesblock_forward`` skips stage A."""
    call = StageA.checked(stage_a)
    lib = _lib.load()
    B = med.shape[0]
    dev = med.device
    nparts = 1 if psum.dim() == 1 else psum.shape[0]     # (with ``xch`` the parts are the exchange buffer's slots)
    desc = torch.empty(DESC_INTS, dtype=torch.int32, device=dev)
    amps = torch.empty(B, FTN_KMAX, dtype=torch.float32, device=dev)
    wts = torch.empty(B, FTN_KMAX, dtype=torch.float32, device=dev)
    mg, pxb = _selector_bounds(lib, L, k, pmax, min_thr)
    sel = Selection(desc, amps, wts, mg, pxb)
    fin = (_ptr(psum), nparts, int(b_total), _ptr(med), B, L, int(k), int(pmax), int(min_thr), int(act_dtype),
           int(max_unique or 0), float(log_base or 0.0), _ptr(desc), _ptr(amps), _ptr(wts))
    if call is not None and (call.ws is not None or fuse_stage_a(call.plan)):
        x = None                                         # stage A is in the workspace already
        if call.ws is None:
            x, call.ws = _ptr(call.x), _workspace(dev, _workspace_bytes(lib, call.plan, B, L, mg, pxb))
        check(lib.ftn_period_finalize_stage_a(*fin, x, C.byref(call.plan), _ptr(call.wblob), mg, pxb, _ptr(call.ws),
                                              call.ws.numel(), _stream(dev), _ptr_or_null(call.range_flag), xch),
              "ftn_period_finalize_stage_a")
        sel.stage_a = call
        return sel
    check(lib.ftn_period_finalize(*fin, _stream(dev), xch), "ftn_period_finalize")
    return sel


def selection_from_host(desc_host: FtnDesc, weights: torch.Tensor, device: torch.device) -> Selection:
    """Upload a host-built descriptor + [B,G] group weights (stub selectors / env flags)."""
    import numpy as np

    raw = np.frombuffer(bytes(desc_host), dtype=np.int32).copy()
    desc = torch.from_numpy(raw).to(device)
    B, G = weights.shape
    w = torch.zeros(B, FTN_KMAX, dtype=torch.float32, device=device)
    w[:, :G] = weights.to(device=device, dtype=torch.float32)
    sel = Selection(desc, w, w, max(1, int(desc_host.n_groups)), max(1, int(desc_host.total_px)))
    sel._host = desc_host
    return sel


# ------------------------------------------------------------------ kernel forms
_SPECTRUM_FORMS = ("k_spectrum", "k_spectrum_row", "k_spectrum_rowq", "k_spectrum_rowq_tiled")


def spectrum_form(B: int, L: int, C: int, x_misalign: int = 0, scratch: bool = True) -> Tuple[str, bool]:
    """The kernel ``ftn_period_spectrum`` runs for this shape (host-only query; ``scratch``: the caller passes the
    scratch buffer, as ``spectrum`` does) and whether it reads x with 16-byte vector loads."""
    f = _form("ftn_period_spectrum_form", B, L, C, x_misalign, bool(scratch))
    return _SPECTRUM_FORMS[f & 3], bool(f & 4)


_STAGE_C = {0: "k_mlp", 1: "k_pw_chain", 2: "k_mlp_bf<{ns}>", 3: "k_mlp_bf_u1<{ns}>", 4: "k_mlp_bf_c128<{ns}>",
            5: "k_mlp_pos64<{ns}>", 6: "k_mlp_pos128<{ns}>"}
_STAGE_E = {0: "k_out", 1: "k_out_fast", 2: "k_out_h<{ns}>", 3: "k_out_merged"}


def timesblock_forms(plan: FtnPlan, B: int, L: int, act_dtype: int = 0, x_misalign: int = 0) -> Dict[str, object]:
    """The kernel form each stage of ``timesblock_forward`` takes (``ftn_timesblock_forms``, host-only): the
    library dispatches through the same function, so this is what runs.  Stage names carry the template arguments
    that vary (activation pieces ``NS``, conv tiles); ``act`` is the ``ACT`` argument every stage shares."""
    lib = _lib.load()
    f = _lib.FtnForms()
    check(lib.ftn_timesblock_forms(C.byref(plan), int(B), int(L), int(act_dtype), int(x_misalign), C.byref(f)),
          "ftn_timesblock_forms")
    ns = f.nsplit
    if f.mode != 0:
        stage_a = "k_embed"
        conv = "k_conv"
    else:
        stage_a = f"k_pw<1,{f.stage_a_epi}>"
        conv = ("k_conv", f"k_conv_bf<{f.conv_n},{ns}>", f"k_conv_bf_fast<{ns},{f.conv_n}>")[f.conv]
    return {"act": "relu" if f.act == 1 else "gelu", "xvec": bool(f.xvec), "yvec": bool(f.yvec), "A": stage_a,
            "conv": conv, "C": _STAGE_C[f.stage_c].format(ns=ns), "r_keeps_x": bool(f.r_keeps_x),
            "r_summed": bool(f.r_summed), "E": _STAGE_E[f.stage_e].format(ns=ns), "half_round": bool(f.half_round)}


def _wide(D: int) -> bool:
    """d_model beyond the narrow shell kernels: the ``ftn_*_wide_*`` entry points (128 < D <= 512) take the call."""
    return int(D) > 128


def _shell_entry(narrow: str, D: int, kind: str = "") -> str:
    """The shell entry point that takes d_model D: ``narrow`` (``ftn_<op>_<what>``) up to 128, its ``ftn_<op>_wide_<what>``
    twin beyond; ``kind`` is the norm suffix of the embedding entries (``""`` or ``"_rms"``)."""
    if _wide(D):
        op, what = narrow[len("ftn_"):].split("_", 1)
        narrow = f"ftn_{op}_wide_{what}"
    return narrow + kind


def _embed_form_name(f: int) -> str:
    no, rt = (f >> 4) & 15, (f >> 8) & 15
    return f"k_embed_in_bf<{no},{rt}>" if f & 1 else f"k_embed_in<{no},{'true' if f & 2 else 'false'}>"


def embed_form_of(N: int, D: int, x_bstride: int = 0, x_misalign: int = 0, w_misalign: int = 0) -> str:
    """The kernel ``ftn_embed_forward`` / ``ftn_embed_rows_strided`` run for a window of N series into d_model D with
    this batch stride (elements) and these byte offsets of x and W from a 16-byte boundary (``ftn_embed_form``,
    host-only: the launch dispatches through the same function, switches included).  D <= 128."""
    f = _form("ftn_embed_form", N, D, x_bstride, x_misalign, w_misalign)
    return _embed_form_name(f)


def embed_wide_form_of(N: int, D: int, x_bstride: int = 0, x_misalign: int = 0, w_misalign: int = 0) -> str:
    """``embed_form_of`` for 128 < D <= 512 (``ftn_embed_wide_form``): ``k_embed_wide_bf<NO,RT,VEC>``."""
    f = _form("ftn_embed_wide_form", N, D, x_bstride, x_misalign, w_misalign)
    return f"k_embed_wide_bf<{(f >> 4) & 15},{(f >> 8) & 15},{'true' if f & 2 else 'false'}>"


def embed_form_at(N: int, D: int, x_bstride: int = 0, x_misalign: int = 0, w_misalign: int = 0) -> str:
    """The kernel ``embed_forward`` / ``embed_rows_strided`` run at any d_model they take: the narrow query up to 128,
    the wide one beyond."""
    return (embed_wide_form_of if _wide(D) else embed_form_of)(N, D, x_bstride, x_misalign, w_misalign)


def embed_form(window: torch.Tensor, weight: torch.Tensor) -> str:
    """The kernel ``embed_forward(window, weight, ...)`` / ``embed_rows_strided(window, weight, ...)`` runs."""
    B, _, N = window.shape
    return embed_form_at(N, weight.shape[0], window.stride(0) if B > 1 else 0, _ptr(window) & 15, _ptr(weight) & 15)


def head_form_of(N: int, D: int, tail_bstride: int = 0, late_bstride: int = 0, misalign_or: int = 0) -> Tuple[str, int]:
    """The kernel ``ftn_head_forward`` runs (``ftn_head_form``, host-only) and the cap on its ``gridDim.y``: the
    row loop of a workgroup iterates when ``rows > 64 * cap``.  D <= 128."""
    f = _form("ftn_head_form", N, D, tail_bstride, late_bstride, misalign_or)
    p0, p1, cap = (f >> 4) & 15, (f >> 8) & 15, f >> 16
    return (f"k_head_bf<{p0},{p1}>" if f & 1 else f"k_head<{p0},{'true' if f & 2 else 'false'}>"), cap


def head_wide_form_of(N: int, D: int, tail_bstride: int = 0, late_bstride: int = 0,
                      misalign_or: int = 0) -> Tuple[str, int]:
    """``head_form_of`` for 128 < D <= 512 (``ftn_head_wide_form``): ``k_head_wide_bf<NT>`` and its cap, or
    ``("k_head_wide_f32", 0)`` for operands that are not vectorisable (a grid-stride kernel: no cap)."""
    f = _form("ftn_head_wide_form", N, D, tail_bstride, late_bstride, misalign_or)
    return (f"k_head_wide_bf<{(f >> 4) & 15}>", f >> 16) if f & 1 else ("k_head_wide_f32", 0)


def head_form_at(N: int, D: int, tail_bstride: int = 0, late_bstride: int = 0, misalign_or: int = 0) -> Tuple[str, int]:
    """The kernel ``head_forward`` runs at any d_model it takes."""
    return (head_wide_form_of if _wide(D) else head_form_of)(N, D, tail_bstride, late_bstride, misalign_or)


def head_form(hidden: torch.Tensor, w_mu: torch.Tensor, tail: torch.Tensor, late=None) -> Tuple[str, int]:
    """``head_form_at`` for the tensors ``head_forward`` would be given (its outputs are fresh, aligned tensors)."""
    B = hidden.shape[0]
    mis = (_ptr(tail) | (_ptr(late) if late is not None else 0)) & 15
    return head_form_at(w_mu.shape[0], hidden.shape[2], tail.stride(0) if B > 1 else 0, _batch_stride(late, B), mis)


def _timeproj_form_name(f: int, row: str) -> str:
    return f"k_timeproj_bf<{(f >> 4) & 15},{'true' if f & 2 else 'false'}>" if f & 1 else row


def timeproj_form_of(L: int, S: int, D: int, wt_misalign: int = 0) -> str:
    """The kernel ``ftn_timeproj_forward`` runs for an ``L -> S`` projection at d_model D with W_t at this byte
    offset from a 16-byte boundary (``ftn_timeproj_form``, host-only: the launch dispatches through the same
    function): ``k_timeproj_row`` for S == 1, else ``k_timeproj_bf<NST,WV>``.  D <= 128."""
    return _timeproj_form_name(_form("ftn_timeproj_form", L, S, D, wt_misalign), "k_timeproj_row")


def timeproj_wide_form_of(L: int, S: int, D: int, wt_misalign: int = 0) -> str:
    """``timeproj_form_of`` for 128 < D <= 512 (``ftn_timeproj_wide_form``): ``k_timeproj_row_wide`` for S == 1, else
    the same ``k_timeproj_bf<NST,WV>``."""
    return _timeproj_form_name(_form("ftn_timeproj_wide_form", L, S, D, wt_misalign), "k_timeproj_row_wide")


def timeproj_form_at(L: int, S: int, D: int, wt_misalign: int = 0) -> str:
    """The kernel ``timeproj_forward`` runs at any d_model it takes."""
    return (timeproj_wide_form_of if _wide(D) else timeproj_form_of)(L, S, D, wt_misalign)


def timeproj_form(seq: torch.Tensor, wt: torch.Tensor) -> str:
    """The kernel ``timeproj_forward(seq, wt, bt)`` runs."""
    return timeproj_form_at(seq.shape[1], wt.shape[0], seq.shape[2], _ptr(wt) & 15)


# ------------------------------------------------------------------ conv path
MAX_ROWS_PER_PASS = 65535


def selector_bounds(L: int, k: int, pmax: int, min_thr: int) -> Tuple[int, int]:
    """``(max_groups, px_bound)`` of the selections ``finalize`` makes for this selector configuration."""
    return _selector_bounds(_lib.load(), L, k, pmax, min_thr)


def rows_per_pass(plan: FtnPlan, L: int, max_groups: int, px_bound: int, ws_cap_bytes: int = 0) -> int:
    """The largest legal ``rows_per_pass`` whose workspace is at most ``ws_cap_bytes`` (0 = no cap): host-only
    (``ftn_timesblock_rows_per_pass``).  0 when one row does not fit."""
    return int(_lib.load().ftn_timesblock_rows_per_pass(C.byref(plan), int(L), int(max_groups), int(px_bound),
                                                        int(ws_cap_bytes)))


def timesblock_forward(x: torch.Tensor, plan: FtnPlan, wblob: torch.Tensor, sel: Selection,
                       norm=None, act_dtype: int = 0, range_flag: Optional[torch.Tensor] = None,
                       rows_per_pass: Optional[int] = None) -> torch.Tensor:
    """``norm=(gamma, beta, eps)`` appends the model's per-block ``LayerNorm(x + (y - x))``
    (reference :2050-2058) to the same call.  ``range_flag``: see ``new_range_flag``.

    ``rows_per_pass`` (None: one pass, B <= 65535): stages A-F run in passes of that many rows over the one
    selection, through a workspace sized for one pass (the ``_rows`` entry points); same bits as one pass."""
    lib = _lib.load()
    B, L, _ = x.shape
    rows = None if rows_per_pass is None else int(rows_per_pass)
    if rows is not None and not 1 <= rows <= MAX_ROWS_PER_PASS:
        raise ValueError(f"rows_per_pass={rows} outside [1, {MAX_ROWS_PER_PASS}]")
    n = B if rows is None else min(B, rows)                  # rows of a pass
    need = _workspace_bytes(lib, plan, n, L, sel.max_groups, sel.px_bound)
    # the selector's finalize launch may have run stage A for THIS x and plan into a workspace it allocated: that
    # serves one forward (a second one on the same selection runs stage A itself, as the range guard's repair does)
    call, sel.stage_a = sel.stage_a, None
    if call is not None:
        if n < B:
            raise RuntimeError("selection carries a fused stage A, which serves a single pass only")
        if call.x.data_ptr() != x.data_ptr() or C.addressof(call.plan) != C.addressof(plan) or call.ws.numel() < need:
            raise RuntimeError("selection carries stage A of a different input or plan")
    ws = _workspace(x.device, need) if call is None else call.ws
    flags = 0 if call is None else 1                         # FTN_FWD_STAGE_A_DONE
    y = torch.empty_like(x)
    entry = "ftn_timesblock_forward" + ("" if norm is None else "_norm") + ("" if rows is None else "_rows")
    mid = (int(act_dtype), flags) if norm is None else (flags, *_norm_args(norm))
    check(getattr(lib, entry)(_ptr(x), _ptr(y), B, L, C.byref(plan), _ptr(wblob), _ptr(sel.desc), _ptr(sel.weights),
                              sel.max_groups, sel.px_bound, *mid, _ptr(ws), ws.numel(), _stream(x.device),
                              _ptr_or_null(range_flag), *(() if rows is None else (rows,))), entry)
    return y


def residual_layernorm(x: torch.Tensor, new: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor,
                       eps: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """LayerNorm over the last axis of ``x + (new - x)`` (fp32, contiguous).  ``out`` may be ``new`` (in place)."""
    lib = _lib.load()
    Cc = x.shape[-1]
    if out is None:
        out = torch.empty_like(x)
    elif out.shape != x.shape or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("out must be contiguous fp32 of x's shape")
    check(lib.ftn_residual_layernorm(_ptr(x), _ptr(new), _ptr(out), x.numel() // Cc, Cc, _ptr(gamma), _ptr(beta),
                                     float(eps), _stream(x.device)), "ftn_residual_layernorm")
    return out


# ------------------------------------------------------------------ model shell
def head_forward(hidden: torch.Tensor, w_mu: torch.Tensor, b_mu: torch.Tensor, w_sigma: torch.Tensor,
                 b_sigma: torch.Tensor, tail: torch.Tensor, hist: int, late, floor_vec, floor_scalar: float):
    """Fused rate / dispersion heads.  ``hidden`` [B,S,D] contiguous fp32; ``tail`` a (possibly strided
    along the batch) view [B,hist,N] of the input window; ``late`` None or contiguous [1|B,S,N].
    Returns ``(rate, dispersion, bad_flag)``; ``bad_flag`` is a 1-element int32 device tensor."""
    lib = _lib.load()
    B, S, D = hidden.shape
    N = w_mu.shape[0]
    if tail.stride(2) != 1 or tail.stride(1) != N or tail.shape != (B, hist, N):
        raise ValueError("tail must be a [B, hist, N] view with contiguous rows")
    dev = hidden.device
    rate = torch.empty(B, S, N, dtype=torch.float32, device=dev)
    disp = torch.empty(B, S, N, dtype=torch.float32, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    if late is not None and (late.shape[-2:] != (S, N) or not late.is_contiguous()):
        raise ValueError("late bias must be contiguous [1|B, S, N]")
    entry = _shell_entry("ftn_head_forward", D)
    check(getattr(lib, entry)(_ptr(hidden), B * S, S, D, N, _ptr(w_mu), _ptr(b_mu), _ptr(w_sigma), _ptr(b_sigma),
                              _ptr(tail), tail.stride(0) if B > 1 else 0, int(hist),
                              _ptr_or_null(late), _batch_stride(late, B), _ptr_or_null(floor_vec), float(floor_scalar),
                              _ptr(rate), _ptr(disp), _ptr(bad), _stream(dev)), entry)
    return rate, disp, bad


def _store_rows(who: str, rows, seq: torch.Tensor) -> torch.Tensor:
    """The row list of a row-mapped call: a contiguous int64 vector of at least one entry beside the store ``seq``."""
    if (not isinstance(rows, torch.Tensor) or rows.dtype != torch.int64 or rows.dim() != 1 or rows.numel() < 1
            or rows.device != seq.device or not rows.is_contiguous()):
        raise ValueError(f"{who}: rows must be a contiguous int64 vector of at least one entry beside seq")
    return rows


def timeproj_forward(seq: torch.Tensor, wt: torch.Tensor, bt: torch.Tensor, rows=None) -> torch.Tensor:
    """``hidden[b] = wt @ seq[b] + bt[:, None]``: ``seq`` [B,L,D] contiguous fp32, ``wt`` [S,L] with contiguous rows
    (a row slice of a taller weight is fine), ``bt`` [S].  Returns [B,S,D].  Row b of the result does not depend on
    B or on which rows share the call.  ``rows`` (int64 ``[B]`` on the device): ``seq`` is an item store
    ``[n_items, L, D]`` read in place, row b of the result comes from item ``rows[b]`` (clamped into the store; the
    ``ftn_timeproj_*forward_rows`` entries) and has the bits of the plain call on ``seq[rows]``."""
    lib = _lib.load()
    if seq.dim() != 3 or wt.dim() != 2 or bt.dim() != 1:
        raise ValueError("timeproj_forward takes seq [B, L, D], wt [S, L] and bt [S]")
    B, L, D = seq.shape
    if rows is not None:
        n_items, B = B, _store_rows("timeproj_forward", rows, seq).numel()
    S = wt.shape[0]
    if wt.shape[1] != L or bt.shape[0] != S:
        raise ValueError(f"wt {tuple(wt.shape)} / bt {tuple(bt.shape)} do not project seq {tuple(seq.shape)}")
    if any(t.dtype != torch.float32 or not t.is_cuda for t in (seq, wt, bt)):
        raise ValueError("timeproj_forward takes fp32 device tensors")
    if not seq.is_contiguous() or (S > 1 and wt.stride(0) != L) or (L > 1 and wt.stride(1) != 1) or \
            (S > 1 and bt.stride(0) != 1):
        raise ValueError("seq must be contiguous, wt rows contiguous with stride L, bt contiguous")
    hidden = torch.empty(B, S, D, dtype=torch.float32, device=seq.device)
    entry = _shell_entry("ftn_timeproj_forward", D) + ("" if rows is None else "_rows")
    mapped = () if rows is None else (n_items, _ptr(rows))
    check(getattr(lib, entry)(_ptr(seq), *mapped, B, L, D, _ptr(wt), _ptr(bt), S, _ptr(hidden), _stream(seq.device)),
          entry)
    return hidden


def embed_forward(window: torch.Tensor, weight: torch.Tensor, add, norm=None) -> torch.Tensor:
    """``window`` [B,L,N] fp32 view with contiguous rows; ``weight`` [D,N]; ``add`` None or contiguous
    [1|B,L,D]; ``norm`` None, ``(gamma, beta, eps)`` of a LayerNorm or ``(gamma, beta, eps, "rms")`` of an RMS norm.
    Returns [B,L,D]."""
    lib = _lib.load()
    B, L, N = window.shape
    D = weight.shape[0]
    kind, norm = _embed_norm(norm)
    if window.stride(2) != 1 or window.stride(1) != N:
        raise ValueError("window rows must be contiguous")
    if add is not None and (add.shape[-2:] != (L, D) or not add.is_contiguous()):
        raise ValueError("add must be contiguous [1|B, L, D]")
    out = torch.empty(B, L, D, dtype=torch.float32, device=window.device)
    entry = _shell_entry("ftn_embed_forward", D, kind)
    check(getattr(lib, entry)(_ptr(window), window.stride(0) if B > 1 else 0, B, L, N, _ptr(weight), D,
                              _ptr_or_null(add), _batch_stride(add, B), *_norm_args(norm),
                              _ptr(out), _stream(window.device)), entry)
    return out


def embed_rows_strided(x: torch.Tensor, weight: torch.Tensor, out: torch.Tensor, slot: int) -> None:
    """``x W^T`` of ``x`` [B,L,N] (fp32 view with contiguous rows) into rows ``slot .. slot+L-1`` of ``out``
    [B,Lr,D] (contiguous fp32), no add, no norm: the GEMM of ``embed_forward`` row for row."""
    lib = _lib.load()
    B, L, N = x.shape
    D = weight.shape[0]
    if x.stride(2) != 1 or x.stride(1) != N:
        raise ValueError("x rows must be contiguous")
    if (out.dim() != 3 or out.shape[0] != B or out.shape[2] != D or not out.is_contiguous()
            or out.dtype != torch.float32 or not 0 <= slot <= out.shape[1] - L):
        raise ValueError("out must be contiguous fp32 [B, Lr, D] with room for L rows from slot")
    entry = _shell_entry("ftn_embed_rows_strided", D)
    check(getattr(lib, entry)(_ptr(x), x.stride(0) if B > 1 else 0, B, L, N, _ptr(weight), D,
                              _ptr(out) + 4 * slot * D, out.stride(0), _stream(x.device)), entry)


def embed_ring(V: torch.Tensor, head: int, add, norm=None) -> torch.Tensor:
    """``out[b, t] = V[b, (head + t) % L] + add[b?, t]`` (+ LayerNorm ``norm = (gamma, beta, eps)`` or RMS norm
    ``(gamma, beta, eps, "rms")``) with ``embed_forward``'s epilogue arithmetic.  ``V`` contiguous fp32 [B,L,D];
    ``add`` None or contiguous [1|B,L,D]."""
    lib = _lib.load()
    B, L, D = V.shape
    kind, norm = _embed_norm(norm)
    if not V.is_contiguous() or V.dtype != torch.float32:
        raise ValueError("V must be contiguous fp32 [B, L, D]")
    if add is not None and (add.dim() != 3 or add.shape[-2:] != (L, D) or add.shape[0] not in (1, B)
                            or not add.is_contiguous()):
        raise ValueError("add must be contiguous [1|B, L, D]")
    out = torch.empty(B, L, D, dtype=torch.float32, device=V.device)
    entry = _shell_entry("ftn_embed_ring", D, kind)
    check(getattr(lib, entry)(_ptr(V), B, L, D, int(head), _ptr_or_null(add), _batch_stride(add, B), *_norm_args(norm),
                              _ptr(out), _stream(V.device)), entry)
    return out


# ------------------------------------------------------------------ context front end
def _f32(t):
    """An optional parameter / operand as the context kernels read it: detached, contiguous fp32."""
    if t is None:
        return None
    t = t.detach()
    return t if t.dtype == torch.float32 and t.is_contiguous() else t.float().contiguous()


def _rows_view(t: torch.Tensor, width: int) -> torch.Tensor:
    """``t`` [.., n, width] with contiguous rows (any batch stride), copied only when its rows are not."""
    ok = (width == 1 or t.stride(-1) == 1) and (t.shape[-2] == 1 or t.stride(-2) == width)
    return t if ok else t.contiguous()


def _out_like(who: str, out, shape, device) -> torch.Tensor:
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=device)
    if out.shape != shape or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError(f"{who}: out must be a contiguous fp32 tensor of shape {tuple(shape)}")
    return out


def context_rows_form_of(F: int, Ws: int, Ed: int, R: int = 0, steps: int = 0) -> Tuple[int, int, int]:
    """``(context slots of a lane, static slots of a lane, passes of the late head)`` of ``ftn_context_rows``."""
    f = _form("ftn_context_rows_form", F, Ws, Ed, R, steps)
    return f & 15, (f >> 4) & 15, (f >> 8) & 255


def context_rows(Bc: int, N: int, context_norm, static=None, static_proj=None, static_norm=None, ids=None, table=None,
                 coeff=None, proj=None, late=None, want_rows: bool = True, out=None):
    """One launch for everything that depends on a series row only (``ftn_context_rows``).

    ``static`` fp32 [N, F] or [Bc, N, F] with ``static_proj = (W_s, b_s)`` and ``static_norm = (gamma, beta, eps)``
    or None; ``ids`` int64 [N] or [1|Bc, N] with ``table`` [V, Ed]; ``context_norm = (gamma, beta, eps)``;
    ``coeff = (W_c, b_c)``, ``proj = (w_p, b_p)``, ``late = ((gamma, beta, eps), W_l, b_l, gate)`` select the optional
    outputs.  Returns ``(rows [Bc, N, ctx] or None, coeff [Bc, N, R] or None, cbias [Bc, N] or None,
    late [Bc, steps, N] or None)``; ``out``: four contiguous fp32 tensors (or None) to write these into instead of
    fresh ones."""
    lib = _lib.load()
    p = _lib.FtnContextParams()
    keep = []

    def put(name, t):
        t = _f32(t)
        keep.append(t)
        setattr(p, name, _ptr_or_null(t))
        return t

    dev = None
    st_ptr = ids_ptr = None
    st_bs = ids_bs = 0
    if static is not None:
        w_s = put("w_s", static_proj[0])
        put("b_s", static_proj[1])
        p.Ws, p.F = int(w_s.shape[0]), int(w_s.shape[1])
        if static.dtype != torch.float32 or static.shape[-2:] != (N, p.F) or static.dim() not in (2, 3):
            raise ValueError(f"context_rows: static must be fp32 [N, F] or [Bc, N, F], got {tuple(static.shape)}")
        static = _rows_view(static.detach(), p.F)
        if static.dim() == 3 and static.shape[0] not in (1, Bc):
            raise ValueError("context_rows: static batch dimension does not match Bc")
        st_bs = static.stride(0) if static.dim() == 3 and static.shape[0] > 1 else 0
        st_ptr, dev = _ptr(static), static.device
        if static_norm is not None:
            put("sn_g", static_norm[0])
            put("sn_b", static_norm[1])
            p.sn_eps = float(static_norm[2])
    if ids is not None:
        tab = put("emb", table)
        p.V, p.Ed = int(tab.shape[0]), int(tab.shape[1])
        if ids.dtype != torch.int64 or ids.shape[-1] != N or ids.dim() not in (1, 2):
            raise ValueError(f"context_rows: ids must be int64 [N] or [1|Bc, N], got {tuple(ids.shape)}")
        ids = ids.detach()
        if N > 1 and ids.stride(-1) != 1:
            ids = ids.contiguous()
        if ids.dim() == 2 and ids.shape[0] not in (1, Bc):
            raise ValueError("context_rows: ids batch dimension does not match Bc")
        ids_bs = ids.stride(0) if ids.dim() == 2 and ids.shape[0] > 1 else 0
        ids_ptr, dev = _ptr(ids), ids.device
    if dev is None:
        raise ValueError("context_rows: neither static features nor ids")
    ctx = p.Ws + p.Ed
    put("cn_g", context_norm[0])
    put("cn_b", context_norm[1])
    p.cn_eps = float(context_norm[2])
    outs = (None,) * 4 if out is None else tuple(out)
    new = lambda i, *shape: _out_like("context_rows", outs[i], shape, dev)
    rows = new(0, Bc, N, ctx) if want_rows else None
    coeff_out = cbias_out = late_out = None
    if coeff is not None:
        w_c = put("w_c", coeff[0])
        put("b_c", coeff[1])
        p.R = int(w_c.shape[0])
        coeff_out = new(1, Bc, N, p.R)
    if proj is not None:
        put("w_p", proj[0])
        put("b_p", proj[1])
        cbias_out = new(2, Bc, N)
    if late is not None:
        (g, b, eps), w_l, b_l, gate = late
        put("ln_g", g)
        put("ln_b", b)
        p.ln_eps = float(eps)
        w_l = put("w_l", w_l)
        put("b_l", b_l)
        put("gate", gate)
        p.steps = int(w_l.shape[0])
        late_out = new(3, Bc, p.steps, N)
    check(lib.ftn_context_rows(C.byref(p), st_ptr, st_bs, ids_ptr, ids_bs, int(Bc), int(N), _ptr_or_null(rows),
                               _ptr_or_null(coeff_out), _ptr_or_null(cbias_out), _ptr_or_null(late_out), _stream(dev)),
          "ftn_context_rows")
    return rows, coeff_out, cbias_out, late_out


def context_through_weight(coeff, cbias, w: torch.Tensor, out=(None, None)):
    """``(q_coeff [Bc, R, D] or None, q_bias [Bc, D] or None)``: ``coeff`` [Bc, N, R] and ``cbias`` [Bc, N] (either may
    be None) contracted over the series with ``w`` [D, N], whose rows may be a column slice of a wider weight."""
    lib = _lib.load()
    coeff, cbias = _f32(coeff), _f32(cbias)
    ref = coeff if coeff is not None else cbias
    if ref is None:
        raise ValueError("context_through_weight: neither coefficients nor bias")
    Bc, N = int(ref.shape[0]), int(ref.shape[1])
    R = int(coeff.shape[2]) if coeff is not None else 0
    if w.dim() != 2 or w.shape[1] != N or w.dtype != torch.float32 or (cbias is not None and cbias.shape != (Bc, N)):
        raise ValueError("context_through_weight: w must be fp32 [D, N] for coeff [Bc, N, R] / cbias [Bc, N]")
    w = w.detach()
    if N > 1 and w.stride(1) != 1:
        w = w.contiguous()
    D = int(w.shape[0])
    ldw = w.stride(0) if D > 1 else N
    q_coeff = _out_like("context_through_weight", out[0], (Bc, R, D), w.device) if coeff is not None else None
    q_bias = _out_like("context_through_weight", out[1], (Bc, D), w.device) if cbias is not None else None
    check(lib.ftn_context_through_weight(_ptr_or_null(coeff), _ptr_or_null(cbias), Bc, N, R, _ptr(w), max(ldw, N), D,
                                         _ptr_or_null(q_coeff), _ptr_or_null(q_bias), _stream(w.device)),
          "ftn_context_through_weight")
    return q_coeff, q_bias


def embed_add_form_of(D: int, q_coeff_bstride: int = 0, q_bias_bstride: int = 0, misalign_or: int = 0) -> str:
    f = _form("ftn_embed_add_form", D, q_coeff_bstride, q_bias_bstride, misalign_or)
    return f"k_embed_add<{(f >> 4) & 15},{'true' if f & 2 else 'false'}>"


def embed_add(L: int, D: int, device, pos=None, mark=None, time=None, aux=None, b_v=None, basisc=None, scale=None,
              q_coeff=None, q_bias=None, out=None) -> torch.Tensor:
    """``add`` [Ba, L, D] of the embedding entry points in one pass (``ftn_embed_add``): ``pos`` [L, D] with the value
    bias ``b_v`` (+ ``mark`` [B, L, T] through ``time = (W_t, b_t)``; ``aux = (gamma, beta, eps, gate)`` in the
    "decoupled" mode), then ``scale * basisc @ q_coeff`` and ``q_bias`` (``context_through_weight``).  Ba is 1 when
    nothing has more than one batch row (a mark with batch stride 0 counts as one row)."""
    lib = _lib.load()
    p = _lib.FtnEmbedAddParams()
    keep = []

    def put(name, t):
        t = _f32(t)
        keep.append(t)
        setattr(p, name, _ptr_or_null(t))
        return t

    Bm = 1
    mark_ptr, mark_bs = None, 0
    if pos is not None:
        if pos.shape != (L, D):
            raise ValueError(f"embed_add: pos must be [L, D] = {(L, D)}, got {tuple(pos.shape)}")
        put("pos", pos)
        put("b_v", b_v)
        if mark is not None:
            w_t = put("w_t", time[0])
            put("b_t", time[1])
            p.T = int(w_t.shape[1])
            if mark.dim() != 3 or mark.shape[1:] != (L, p.T) or mark.dtype != torch.float32:
                raise ValueError(f"embed_add: mark must be fp32 [B, L, {p.T}], got {tuple(mark.shape)}")
            mark = _rows_view(mark.detach(), p.T)
            if mark.shape[0] > 1 and mark.stride(0) != 0:
                Bm, mark_bs = int(mark.shape[0]), mark.stride(0)
            mark_ptr = _ptr(mark)
        if aux is not None:
            put("aux_g", aux[0])
            put("aux_b", aux[1])
            p.aux_eps = float(aux[2])
            put("gate", aux[3])
    Bq = 1
    R = 0
    if q_coeff is not None:
        R = int(q_coeff.shape[1])
        Bq = int(q_coeff.shape[0])
        put("basisc", basisc)
        put("scale", scale)
        if keep[-2].shape != (L, R):
            raise ValueError("embed_add: basisc must be [L, R]")
    if q_bias is not None:
        Bq = int(q_bias.shape[0])
    if Bm > 1 and Bq > 1 and Bm != Bq:
        raise ValueError(f"embed_add: {Bm} mark rows against {Bq} context rows")
    Ba = max(Bm, Bq)
    out = _out_like("embed_add", out, (Ba, L, D), device)
    check(lib.ftn_embed_add(C.byref(p), mark_ptr, mark_bs, _ptr_or_null(q_coeff), R * D if Bq > 1 else 0, R,
                            _ptr_or_null(q_bias), D if Bq > 1 else 0, Ba, int(L), int(D), _ptr(out), _stream(device)),
          "ftn_embed_add")
    return out


# ------------------------------------------------------------------ row exchange (series-sharded forward)
def rowx_push(src: torch.Tensor, xch) -> None:
    """Store this rank's rows into every destination's buffer (``xch``: ``C.byref`` of an ``FtnRowExchange``).
    ``src`` contiguous fp32: ``[W*R, width]`` for a reduce-scatter, ``[R, width]`` for an all-gather."""
    if src.dtype != torch.float32 or not src.is_contiguous():
        raise ValueError("rowx_push: src must be contiguous fp32")
    check(_lib.load().ftn_rowx_push(_ptr(src), xch, _stream(src.device)), "ftn_rowx_push")


def rowx_reduce(xch, rows: int, L: int, D: int, device: torch.device, add=None, norm=None) -> torch.Tensor:
    """This rank's ``[rows, L, D]`` of the rank-order sum of every rank's pushed partials, ``+ add`` (None, or contiguous
    ``[1|rows, L, D]``), then the LayerNorm ``norm = (gamma, beta, eps)`` over D (optional)."""
    out = torch.empty(rows, L, D, dtype=torch.float32, device=device)
    if add is not None and (add.shape[-2:] != (L, D) or not add.is_contiguous() or add.dtype != torch.float32):
        raise ValueError("rowx_reduce: add must be contiguous fp32 [1|rows, L, D]")
    check(_lib.load().ftn_rowx_reduce(xch, int(L), int(D), _ptr_or_null(add), _batch_stride(add, rows),
                                      *_norm_args(norm), _ptr(out), _stream(device)), "ftn_rowx_reduce")
    return out


def rowx_gather(xch, shape, device: torch.device) -> torch.Tensor:
    """Every rank's pushed rows, row block s from rank s, as a new fp32 tensor of ``shape`` (``[W*R, ...]``)."""
    out = torch.empty(shape, dtype=torch.float32, device=device)
    check(_lib.load().ftn_rowx_gather(xch, _ptr(out), _stream(device)), "ftn_rowx_gather")
    return out


# ------------------------------------------------------------------ scoring
SCORE_PART_BYTES = _lib.SCORE_PART_BYTES


def score_form_of(H: int, N: int, strides=(0, 0, 0), misalign_or: int = 0) -> Tuple[str, int, int]:
    """The kernel ``ftn_score_columns`` runs (``ftn_score_form``, host-only: the launch dispatches through the same
    function): ``("k_score_cols<4>" | "k_score_cols<1>", nseg, seg)`` - the vector form reads 16 bytes per lane and
    needs ``N % 4 == 0``, batch ``strides`` (of y, rate, dispersion, in elements) that are multiples of 4 and
    ``misalign_or == 0``; H is cut into ``nseg`` segments of ``seg`` rows."""
    f = _form("ftn_score_form", H, N, strides[0], strides[1], strides[2], misalign_or)
    return f"k_score_cols<{4 if f & 2 else 1}>", (f >> 4) & 15, f >> 8


def rows_ok(t: torch.Tensor) -> bool:
    """Whether ``t`` [.., H, N] (3-d [B,H,N] or 4-d path-major [P,B,H,N]) has the layout the scoring kernels take: rows
    contiguous and N apart, and every outer stride at least the extent of what lies beneath it."""
    s, (H, N) = t.stride(), t.shape[-2:]
    if (N > 1 and s[-1] != 1) or (H > 1 and s[-2] != N):
        return False
    extent = H * N
    for d in range(t.dim() - 3, -1, -1):
        if t.shape[d] > 1:
            if s[d] < extent:
                return False
            extent += (t.shape[d] - 1) * s[d]
    return True


def _bhn_operands(who: str, operands) -> Tuple[int, int, int]:
    """The preamble of the [B,H,N] wrappers for ``(name, tensor)`` pairs: shapes, then row layout, then dtype and
    device, one device, no empty shape.  Returns ``(B, H, N)``."""
    first = operands[0][0]
    for name, t in operands:
        if not isinstance(t, torch.Tensor) or t.dim() != 3:
            raise ValueError(f"{who}: {name} must be a [B, H, N] tensor")
        if t.shape != operands[0][1].shape:
            raise ValueError(f"{who}: {name} has shape {tuple(t.shape)}, {first} has {tuple(operands[0][1].shape)}")
    for name, t in operands:
        if not rows_ok(t):
            raise ValueError(f"{who}: {name} needs contiguous rows N elements apart, strides {t.stride()}")
    for name, t in operands:
        if t.dtype != torch.float32 or not t.is_cuda:
            raise ValueError(f"{who}: {name} must be an fp32 device tensor, got {t.dtype} on {t.device}")
    if len({t.device for _, t in operands}) != 1:
        raise ValueError(f"{who}: {', '.join(n for n, _ in operands)} must be on one device")
    B, H, N = operands[0][1].shape
    if B < 1 or H < 1 or N < 1:
        raise ValueError(f"{who}: empty shape {(B, H, N)}")
    return B, H, N


def _out_or_fresh(who: str, out, shape, like: torch.Tensor, name: str = "out") -> torch.Tensor:
    """``out`` when it is a contiguous fp32 tensor of ``shape`` beside ``like``, a fresh one when it is None."""
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=like.device)
    if out.dtype != torch.float32 or out.device != like.device or not out.is_contiguous() or tuple(out.shape) != shape:
        raise ValueError(f"{who}: {name} must be contiguous fp32 {shape} beside its operands")
    return out


def _flag_or_fresh(who: str, flag, device, optional: bool = False):
    """``flag`` when it is one int32 on ``device``; for None a fresh zeroed one, or None where it is ``optional``."""
    if flag is None:
        return None if optional else torch.zeros(1, dtype=torch.int32, device=device)
    if (not isinstance(flag, torch.Tensor) or flag.dtype != torch.int32 or flag.numel() != 1 or not flag.is_cuda
            or flag.device != device):
        raise ValueError(f"{who}: flag must be one int32 on the operands' device")
    return flag


def _score_mask(mask, y: torch.Tensor):
    if mask is None:
        return None, 0
    if tuple(mask.shape) != tuple(y.shape) or not mask.is_contiguous() or mask.device != y.device:
        raise ValueError(f"score_columns: mask must be contiguous {tuple(y.shape)} beside y, got "
                         f"{tuple(mask.shape)} strides {mask.stride()} on {mask.device}")
    if mask.dtype in (torch.bool, torch.uint8):
        return mask, 1
    if mask.dtype == torch.float32:
        return mask, 2
    raise ValueError(f"score_columns: mask must be bool, uint8 or fp32, got {mask.dtype}")


def _score_misalign(y, rate, disp, mask, kind, ll) -> int:
    mis = (_ptr(y) | _ptr(rate) | _ptr(disp) | (_ptr(ll) if ll is not None else 0)) & 15
    if kind == 2:
        mis |= _ptr(mask) & 15
    if kind == 1:
        mis |= (_ptr(mask) & 3) << 2
    return mis


def score_form(y, rate, disp, mask=None, ll_out=None) -> Tuple[str, int, int]:
    """``score_form_of`` for the tensors ``score_columns`` is given."""
    B, H, N = y.shape
    _, kind = _score_mask(mask, y)
    strides = [t.stride(0) if B > 1 else 0 for t in (y, rate, disp)]
    return score_form_of(H, N, strides, _score_misalign(y, rate, disp, mask, kind, ll_out))


def score_columns(y: torch.Tensor, rate: torch.Tensor, disp: torch.Tensor, mask=None, eps: float = 1e-8,
                  want_ll: bool = False):
    """One pass of ``k_score_cols`` over ``y``, ``rate``, ``disp`` [B,H,N] (fp32 device tensors or views with
    contiguous rows N elements apart) and an optional contiguous [B,H,N] mask (bool / uint8, or fp32 where nonzero is
    true).  Returns ``(part, ll)``: ``part`` a uint8 tensor of B N ``FtnScorePart`` records, column (b, n) at record
    ``b N + n``; ``ll`` the fp32 per-element log-likelihood (0 where invalid) when ``want_ll``, else None.  Enqueues
    only."""
    lib = _lib.load()
    B, H, N = _bhn_operands("score_columns", (("y", y), ("rate", rate), ("dispersion", disp)))
    mask, kind = _score_mask(mask, y)
    part = torch.empty(B * N * SCORE_PART_BYTES, dtype=torch.uint8, device=y.device)
    ll = torch.empty(B, H, N, dtype=torch.float32, device=y.device) if want_ll else None
    check(lib.ftn_score_columns(_ptr(y), y.stride(0), _ptr(rate), rate.stride(0), _ptr(disp), disp.stride(0),
                                _ptr_or_null(mask), kind, float(eps), B, H, N, _ptr(part), _ptr_or_null(ll),
                                _stream(y.device)), "ftn_score_columns")
    return part, ll


def score_fold(part: torch.Tensor, B: int, N: int, acc: torch.Tensor, err: torch.Tensor, ids=None, order=None,
               seg_start=None) -> None:
    """``acc[slot] += part[b N + n]`` in place (``k_score_fold``), in ascending (b, n) order per slot.  ``acc``: uint8
    storage of ``FtnScorePart`` records, one per slot; ``err``: one int32 whose bit 0 an out-of-range id sets.
    No ids: slot = n.  ``ids`` int64 [N] (distinct): slot = ids[n].  ``order`` int64 [B N] with ``seg_start`` int64
    [n_slots + 1] (the stable argsort of any ids and each slot's first position in it): one owner per slot."""
    lib = _lib.load()
    for name, t in (("part", part), ("acc", acc)):
        if t.dtype != torch.uint8 or not t.is_cuda or not t.is_contiguous() or t.numel() % SCORE_PART_BYTES:
            raise ValueError(f"score_fold: {name} must be contiguous uint8 device storage of FtnScorePart records")
    n_slots = acc.numel() // SCORE_PART_BYTES
    if part.numel() != B * N * SCORE_PART_BYTES:
        raise ValueError(f"score_fold: part holds {part.numel() // SCORE_PART_BYTES} records, B N = {B * N}")
    if err.dtype != torch.int32 or err.numel() != 1 or not err.is_cuda:
        raise ValueError("score_fold: err must be one int32 on the device")
    kind = 0
    if order is not None or seg_start is not None:
        kind = 2
        if ids is not None or order is None or seg_start is None:
            raise ValueError("score_fold: order and seg_start come together, without ids")
        for name, t, n in (("order", order, B * N), ("seg_start", seg_start, n_slots + 1)):
            if t.dtype != torch.int64 or not t.is_cuda or not t.is_contiguous() or t.numel() != n:
                raise ValueError(f"score_fold: {name} must be contiguous int64 [{n}] on the device")
    elif ids is not None:
        kind = 1
        if ids.dtype != torch.int64 or not ids.is_cuda or not ids.is_contiguous() or tuple(ids.shape) != (N,):
            raise ValueError(f"score_fold: ids must be contiguous int64 [{N}] on the device")
    check(lib.ftn_score_fold(_ptr(part), int(B), int(N), kind, _ptr_or_null(ids), _ptr_or_null(order),
                             _ptr_or_null(seg_start), _ptr(acc), n_slots, _ptr(err), _stream(part.device)),
          "ftn_score_fold")


# ------------------------------------------------------------------ head refit
def nb_nll_grad_form_of(B: int, H: int, N: int, strides=(0, 0, 0), misalign_or: int = 0) -> Tuple[str, int]:
    """The kernel ``ftn_nb_nll_grad`` runs (``ftn_nb_nll_grad_form``, host-only) and the workgroups of its grid:
    ``("k_nb_grad<4>" | "k_nb_grad<1>", nparts)`` - the vector form needs ``H N % 4 == 0``, batch ``strides`` that are
    multiples of 4 and ``misalign_or == 0``."""
    f = _form("ftn_nb_nll_grad_form", B, H, N, strides[0], strides[1], strides[2], misalign_or)
    return f"k_nb_grad<{4 if f & 2 else 1}>", f >> 4


def nb_nll_grad_form(y, rate, disp, mask=None, g_rate=None, g_disp=None) -> Tuple[str, int]:
    """``nb_nll_grad_form_of`` for the tensors ``nb_nll_grad`` is given (fresh outputs are aligned)."""
    B, H, N = y.shape
    _, kind = _score_mask(mask, y)
    mis = _score_misalign(y, rate, disp, mask, kind, g_rate) | ((_ptr(g_disp) & 15) if g_disp is not None else 0)
    return nb_nll_grad_form_of(B, H, N, [t.stride(0) if B > 1 else 0 for t in (y, rate, disp)], mis)


def nb_nll_grad(y: torch.Tensor, rate: torch.Tensor, disp: torch.Tensor, mask=None, eps: float = 1e-8,
                scaled: bool = True, g_rate: torch.Tensor | None = None, g_disp: torch.Tensor | None = None):
    """``ftn_nb_nll_grad`` over ``y``, ``rate``, ``disp`` [B,H,N] and an optional mask (the operands of
    ``score_columns``).  Returns ``(words, g_rate, g_disp)``: ``words`` two fp32 on the device, the loss and the scale
    ``-1 / max(valid, 1)``; the gradients of the loss when ``scaled``, else the raw derivatives of the log-likelihood.
    ``g_rate`` / ``g_disp`` may be the caller's (contiguous fp32 [B,H,N]).  Enqueues only."""
    lib = _lib.load()
    B, H, N = _bhn_operands("nb_nll_grad", (("y", y), ("rate", rate), ("dispersion", disp)))
    mask, kind = _score_mask(mask, y)
    g_rate = _out_or_fresh("nb_nll_grad", g_rate, (B, H, N), y, "g_rate")
    g_disp = _out_or_fresh("nb_nll_grad", g_disp, (B, H, N), y, "g_disp")
    need = lib.ftn_nb_nll_grad_workspace(B, H, N)
    if need == 0:
        raise ValueError(f"nb_nll_grad: ftn_nb_nll_grad_workspace rejected the shape {(B, H, N)}")
    workspace = _workspace(y.device, need)
    words = torch.empty(2, dtype=torch.float32, device=y.device)
    check(lib.ftn_nb_nll_grad(_ptr(y), y.stride(0), _ptr(rate), rate.stride(0), _ptr(disp), disp.stride(0),
                              _ptr_or_null(mask), kind, float(eps), B, H, N, _ptr(g_rate), _ptr(g_disp), _ptr(words),
                              _ptr(workspace), workspace.numel(), int(bool(scaled)), _stream(y.device)),
          "ftn_nb_nll_grad")
    return words, g_rate, g_disp


def head_backward_form_of(R: int, N: int, D: int, misalign_or: int = 0) -> Tuple[str, int]:
    """The kernel ``ftn_head_backward`` runs (``ftn_head_backward_form``, host-only) and its row chunks:
    ``("k_headfit_colsum<N>" | "k_headfit_mfma", chunks)`` - the column sums for ``N <= 4`` and a ``hidden`` on the
    16-byte grid."""
    f = _form("ftn_head_backward_form", R, N, D, misalign_or)
    return (f"k_headfit_colsum<{N}>" if f & 15 == _lib.FTN_HEADFIT_COLSUM else "k_headfit_mfma"), f >> 4


def head_fit_forward(hidden: torch.Tensor, w_mu: torch.Tensor, b_mu: torch.Tensor, w_sigma: torch.Tensor,
                     b_sigma: torch.Tensor, tail: torch.Tensor, hist: int, late, floor_vec, floor_scalar: float):
    """``head_forward``'s operands through ``ftn_head_fit_forward``: ``(rate, dispersion, sig_mu, sig_sigma, bad)``
    with ``sig_*`` [B,S,N] softplus' derivative at the two pre-activations."""
    lib = _lib.load()
    B, S, D = hidden.shape
    N = w_mu.shape[0]
    if tail.stride(2) != 1 or tail.stride(1) != N or tail.shape != (B, hist, N):
        raise ValueError("tail must be a [B, hist, N] view with contiguous rows")
    if late is not None and (late.shape[-2:] != (S, N) or not late.is_contiguous()):
        raise ValueError("late bias must be contiguous [1|B, S, N]")
    if not hidden.is_contiguous():
        raise ValueError("hidden must be contiguous [B, S, D]")
    dev = hidden.device
    rate, disp, sig_mu, sig_sg = (torch.empty(B, S, N, dtype=torch.float32, device=dev) for _ in range(4))
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    check(lib.ftn_head_fit_forward(_ptr(hidden), B * S, S, D, N, _ptr(w_mu), _ptr(b_mu), _ptr(w_sigma), _ptr(b_sigma),
                                   _ptr(tail), tail.stride(0) if B > 1 else 0, int(hist), _ptr_or_null(late),
                                   _batch_stride(late, B), _ptr_or_null(floor_vec), float(floor_scalar), _ptr(rate),
                                   _ptr(disp), _ptr(sig_mu), _ptr(sig_sg), _ptr(bad), _stream(dev)),
          "ftn_head_fit_forward")
    return rate, disp, sig_mu, sig_sg, bad


def head_backward(hidden: torch.Tensor, g_rate: torch.Tensor, g_disp: torch.Tensor, sig_mu: torch.Tensor,
                  sig_sigma: torch.Tensor, scale: torch.Tensor, w_mu=None, w_sigma=None, want_hidden: bool = False):
    """``ftn_head_backward``: ``hidden`` [R, D] (or [B,S,D]) with contiguous rows, the raw derivatives and sigmoids
    [R, N] contiguous, ``scale`` one fp32 device word.  Returns ``(dW_mu, db_mu, dW_sigma, db_sigma, d_hidden)``
    (``d_hidden`` None unless ``want_hidden``, which needs both weights).  Enqueues only."""
    lib = _lib.load()
    D = hidden.shape[-1]
    R = hidden.numel() // D
    N = g_rate.numel() // R
    ops = (("g_rate", g_rate), ("g_disp", g_disp), ("sig_mu", sig_mu), ("sig_sigma", sig_sigma))
    if hidden.dtype != torch.float32 or not hidden.is_cuda or hidden.stride(-1) != 1 or (
            hidden.dim() > 1 and not hidden.reshape(R, D).stride(0) == D):
        raise ValueError("head_backward: hidden must be an fp32 device tensor with contiguous rows D apart")
    for name, t in ops:
        if t.dtype != torch.float32 or t.device != hidden.device or not t.is_contiguous() or t.numel() != R * N:
            raise ValueError(f"head_backward: {name} must be contiguous fp32 [{R}, {N}] beside hidden")
    if scale.dtype != torch.float32 or scale.numel() != 1 or scale.device != hidden.device:
        raise ValueError("head_backward: scale must be one fp32 word beside hidden")
    if want_hidden and (w_mu is None or w_sigma is None):
        raise ValueError("head_backward: d_hidden needs both weights")
    dev = hidden.device
    dw_mu, dw_sg = (torch.empty(N, D, dtype=torch.float32, device=dev) for _ in range(2))
    db_mu, db_sg = (torch.empty(N, dtype=torch.float32, device=dev) for _ in range(2))
    d_hidden = torch.empty(R, D, dtype=torch.float32, device=dev).view(hidden.shape) if want_hidden else None
    need = lib.ftn_head_backward_workspace(R, N, D)
    if need == 0:
        raise ValueError(f"head_backward: ftn_head_backward_workspace rejected R={R} N={N} d_model={D}")
    ws = _workspace(dev, need)
    check(lib.ftn_head_backward(_ptr(hidden), R, N, D, _ptr(g_rate), _ptr(g_disp), _ptr(sig_mu), _ptr(sig_sigma),
                                _ptr(scale), _ptr_or_null(w_mu), _ptr_or_null(w_sigma), _ptr(dw_mu), _ptr(db_mu),
                                _ptr(dw_sg), _ptr(db_sg), _ptr_or_null(d_hidden), _ptr(ws), ws.numel(), _stream(dev)),
          "ftn_head_backward")
    return dw_mu, db_mu, dw_sg, db_sg, d_hidden


def timeproj_backward_form_of(B: int, L: int, S: int, D: int, misalign_or: int = 0) -> Tuple[str, int]:
    """The kernel ``ftn_timeproj_backward`` runs (``ftn_timeproj_backward_form``, host-only) and its chunks of batch
    rows: ``("k_timeproj_bwd_mfma", chunks)``.  ``misalign_or``: the OR of ``address & 15`` of seq and d_hidden;
    operands off the 16-byte grid have no form (ValueError, as from the launch)."""
    f = _form("ftn_timeproj_backward_form", B, L, S, D, misalign_or)
    return {_lib.FTN_TIMEPROJ_BWD_MFMA: "k_timeproj_bwd_mfma"}[f & 15], f >> 4


def timeproj_backward(seq: torch.Tensor, d_hidden: torch.Tensor, dw=None, db=None, rows=None):
    """``ftn_timeproj_backward``: ``seq`` [B,L,D] and ``d_hidden`` [B,S,D] contiguous fp32 on one device (16-byte
    aligned, or ValueError).  Returns ``(dW_t [S,L], db_t [S])``, the gradients of ``timeproj_forward``'s ``wt`` and
    ``bt``; ``dw`` / ``db`` may be the caller's (contiguous fp32).  ``rows`` (int64 ``[B]`` on the device): ``seq`` is
    an item store ``[n_items, L, D]`` and batch row b reads item ``rows[b]``, clamped into the store
    (``ftn_timeproj_backward_rows``): the bits of the plain call on ``seq[rows]``.  Enqueues only."""
    lib = _lib.load()
    n_rows = seq.shape[0] if rows is None or seq.dim() < 1 else _store_rows("timeproj_backward", rows, seq).numel()
    if seq.dim() != 3 or d_hidden.dim() != 3 or seq.shape[2] != d_hidden.shape[2] or n_rows != d_hidden.shape[0]:
        raise ValueError("timeproj_backward takes seq [B, L, D] and d_hidden [B, S, D]" if rows is None else
                         "timeproj_backward takes seq [n_items, L, D], rows [B] and d_hidden [B, S, D]")
    for name, t in (("seq", seq), ("d_hidden", d_hidden)):
        if t.dtype != torch.float32 or not t.is_cuda or t.device != seq.device or not t.is_contiguous():
            raise ValueError(f"timeproj_backward: {name} must be a contiguous fp32 device tensor")
    n_items, L, D = seq.shape
    B, S = d_hidden.shape[:2]
    dw = _out_or_fresh("timeproj_backward", dw, (S, L), seq, "dw")
    db = _out_or_fresh("timeproj_backward", db, (S,), seq, "db")
    need = lib.ftn_timeproj_backward_workspace(B, L, S, D)
    if need == 0:
        raise ValueError(f"timeproj_backward: ftn_timeproj_backward_workspace rejected B={B} L={L} S={S} d_model={D}")
    ws = _workspace(seq.device, need)
    if rows is None:
        check(lib.ftn_timeproj_backward(_ptr(seq), _ptr(d_hidden), B, L, S, D, _ptr(dw), _ptr(db), _ptr(ws), ws.numel(),
                                        _stream(seq.device)), "ftn_timeproj_backward")
    else:
        check(lib.ftn_timeproj_backward_rows(_ptr(seq), n_items, _ptr(rows), _ptr(d_hidden), B, L, S, D, _ptr(dw),
                                             _ptr(db), _ptr(ws), ws.numel(), _stream(seq.device)),
              "ftn_timeproj_backward_rows")
    return dw, db


def refit_rows_gather(rows: torch.Tensor, tail: torch.Tensor, y: torch.Tensor, mask=None, late=None, out=None,
                      rows_ok=None, status=None):
    """``ftn_refit_rows_gather``: the batch tensors of a cached refit step from the per-item stores ``tail``
    ``[n_items, hist, N]``, ``y`` ``[n_items, S, N]`` and the optional ``mask`` / ``late`` ``[n_items, S, N]``
    (contiguous fp32 on one device) through ``rows`` (int64 ``[B]`` there).  Returns ``(tail_b, y_b, mask_b, late_b,
    rows_ok, status)``: row b of each batch tensor is row ``rows[b]`` of its store, an index outside the store clamped
    into it; ``rows_ok`` is the clamped list and ``status`` one int32, 4 when an index was outside, else 0 (rewritten
    by every call).  ``out``: the caller's four batch tensors (None for an absent operand), ``rows_ok`` / ``status``
    likewise.  One launch, enqueues only."""
    lib = _lib.load()
    if tail.dim() != 3 or y.dim() != 3 or tail.shape[0] != y.shape[0] or tail.shape[2] != y.shape[2]:
        raise ValueError("refit_rows_gather takes tail [n_items, hist, N] and y [n_items, S, N]")
    n_items, S, N = y.shape
    hist = tail.shape[1]
    stores = [("tail", tail), ("y", y), ("mask", mask), ("late", late)]
    for name, t in stores:
        if t is None:
            continue
        if (t.dtype != torch.float32 or not t.is_cuda or t.device != y.device or not t.is_contiguous()
                or tuple(t.shape) != ((n_items, hist, N) if name == "tail" else (n_items, S, N))):
            raise ValueError(f"refit_rows_gather: {name} must be a contiguous fp32 device tensor of its store's shape")
    B = _store_rows("refit_rows_gather", rows, y).numel()
    out = [None] * 4 if out is None else list(out)
    if len(out) != 4:
        raise ValueError("refit_rows_gather: out is (tail, y, mask, late)")
    outs = []
    for (name, t), o in zip(stores, out):
        if t is None:
            if o is not None:
                raise ValueError(f"refit_rows_gather: an output for {name}, which has no store")
            outs.append(None)
        else:
            outs.append(_out_or_fresh("refit_rows_gather", o, (B,) + tuple(t.shape[1:]), y, name))
    if rows_ok is None:
        rows_ok = torch.empty(B, dtype=torch.int64, device=y.device)
    else:
        _store_rows("refit_rows_gather", rows_ok, y)
        if rows_ok.numel() != B:
            raise ValueError(f"refit_rows_gather: rows_ok must have {B} entries")
    status = _flag_or_fresh("refit_rows_gather", status, y.device)
    check(lib.ftn_refit_rows_gather(_ptr(rows), B, n_items, _ptr(tail), hist * N, _ptr(y), _ptr_or_null(mask),
                                    _ptr_or_null(late), S * N, _ptr(outs[0]), _ptr(outs[1]), _ptr_or_null(outs[2]),
                                    _ptr_or_null(outs[3]), _ptr(rows_ok), _ptr(status), _stream(y.device)),
          "ftn_refit_rows_gather")
    return outs[0], outs[1], outs[2], outs[3], rows_ok, status


# ------------------------------------------------------------------ refit step: clip and AdamW
_REFIT_FORMS = {_lib.FTN_REFIT_ONE: "k_refit_one", _lib.FTN_REFIT_GRID: "k_refit_norm+k_refit_apply"}


def _refit_counts(counts):
    counts = [int(c) for c in counts]
    return len(counts), (C.c_longlong * max(len(counts), 1))(*counts)


def refit_update_form_of(counts, misalign=None) -> Tuple[str, int, int]:
    """The form ``ftn_refit_update`` takes for tensors of ``counts`` elements (``ftn_refit_update_form``, host-only):
    ``("k_refit_one" | "k_refit_norm+k_refit_apply", scalar mask, chunks)``.  ``misalign``: per tensor the OR of
    ``address & 15`` of its parameter, gradient and moments (None: all aligned); bit i of the mask says tensor i is
    moved with scalar accesses.  More than 8 tensors or an empty one is a ValueError, as from the launch."""
    n, arr = _refit_counts(counts)
    mis = None
    if misalign is not None:
        if len(misalign) != n:
            raise ValueError(f"refit_update_form_of: {len(misalign)} misalign values for {n} tensors")
        mis = (C.c_int * max(n, 1))(*(int(v) for v in misalign))
    f = _lib.load().ftn_refit_update_form(n, arr, mis)
    if f < 0:
        check(f, "ftn_refit_update_form")
    return _REFIT_FORMS[f & 15], (f >> 4) & 255, f >> 12


def _refit_record(who: str, params, grads, exp_avg, exp_avg_sq, lr, state, betas, eps, weight_decay, max_norm, skip,
                  range_mask, loss, log):
    """One ``FtnRefitArgs`` record without its workspace, every operand checked: ``(record, device, counts)``."""
    lists = [list(params), list(grads), list(exp_avg), list(exp_avg_sq)]
    n = len(lists[0])
    if any(len(l) != n for l in lists):
        raise ValueError(f"{who}: params, grads, exp_avg and exp_avg_sq must have one length")
    if not 1 <= n <= _lib.FTN_REFIT_MAX_TENSORS:
        raise ValueError(f"{who}: {n} tensors (1..{_lib.FTN_REFIT_MAX_TENSORS} per call)")
    dev = lists[0][0].device
    a = _lib.FtnRefitArgs()
    for i in range(n):
        for name, l in zip(("p", "g", "m", "v"), lists):
            t = l[i]
            if (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda or t.device != dev
                    or not t.is_contiguous() or t.numel() != lists[0][i].numel()):
                raise ValueError(f"{who}: {name}[{i}] must be a contiguous fp32 device tensor of its "
                                 "parameter's size")
            getattr(a, name)[i] = _ptr(t)
        a.n[i] = lists[0][i].numel()
    words = [("lr", lr, torch.float32, 1), ("state", state, torch.int32, 2)]
    words += [(f"skip[{k}]", w, torch.int32, 1) for k, w in enumerate(skip)]
    if loss is not None:
        words.append(("loss", loss, torch.float32, 1))
    for name, t, dtype, count in words:
        if (not isinstance(t, torch.Tensor) or t.dtype != dtype or t.numel() != count or t.device != dev
                or not t.is_contiguous()):
            raise ValueError(f"{who}: {name} must be {count} {dtype} word(s) beside the parameters")
    skip = list(skip)
    if len(skip) > _lib.FTN_REFIT_MAX_SKIP:
        raise ValueError(f"{who}: {len(skip)} skip words (at most {_lib.FTN_REFIT_MAX_SKIP})")
    if log is not None and (log.dtype != torch.float32 or log.device != dev or not log.is_contiguous()
                            or log.dim() != 2 or log.shape[1] != 4 or log.shape[0] < 1):
        raise ValueError(f"{who}: log must be contiguous fp32 [cap >= 1, 4] beside the parameters")
    a.n_tensors, a.n_skip = n, len(skip)
    a.beta1, a.beta2, a.eps, a.weight_decay = float(betas[0]), float(betas[1]), float(eps), float(weight_decay)
    a.max_norm = 0.0 if max_norm is None else float(max_norm)
    a.lr, a.state = _ptr(lr), _ptr(state)
    for k, w in enumerate(skip):
        a.skip[k] = _ptr(w)
    a.range_mask = int(range_mask)
    a.log_cap = 0 if log is None else log.shape[0]
    a.loss, a.log = _ptr_or_null(loss), _ptr_or_null(log)
    return a, dev, [int(a.n[i]) for i in range(n)]


def _refit_workspace(who: str, workspace, dev, need: int) -> torch.Tensor:
    if workspace is None:
        return _workspace(dev, need)
    if workspace.dtype != torch.uint8 or workspace.device != dev or not workspace.is_contiguous():
        raise ValueError(f"{who}: workspace must be contiguous uint8 storage beside the parameters")
    return workspace


def refit_update(params, grads, exp_avg, exp_avg_sq, lr: torch.Tensor, state: torch.Tensor, betas=(0.9, 0.999),
                 eps: float = 1e-8, weight_decay: float = 0.0, max_norm: Optional[float] = None, skip=(),
                 range_mask: int = 0, loss: Optional[torch.Tensor] = None, log: Optional[torch.Tensor] = None,
                 workspace: Optional[torch.Tensor] = None, force_form: Optional[str] = None) -> None:
    """``ftn_refit_update``: clip by the global norm of ``grads`` (``max_norm`` None or <= 0: no clip), then AdamW on
    ``params`` with the moments ``exp_avg`` / ``exp_avg_sq``, in place; up to 8 contiguous fp32 device tensors each.
    ``lr`` one fp32 device word, ``state`` int32 ``[t, calls]`` on the device, ``skip`` int32 device words (bit k of
    ``range_mask``: word k is a block's range word, else a head's ``bad`` word), ``loss`` an optional fp32 word,
    ``log`` an optional contiguous fp32 ``[cap, 4]``.  ``workspace``: uint8 storage of ``ftn_refit_update_workspace``
    bytes (None: from the caching allocator).  ``force_form``: ``"one"`` / ``"grid"``, for tests.  Enqueues only."""
    lib = _lib.load()
    a, dev, counts = _refit_record("refit_update", params, grads, exp_avg, exp_avg_sq, lr, state, betas, eps,
                                   weight_decay, max_norm, skip, range_mask, loss, log)
    if force_form not in (None, "one", "grid"):
        raise ValueError(f"refit_update: force_form {force_form!r} is not 'one', 'grid' or None")
    n, arr = _refit_counts(counts)
    need = lib.ftn_refit_update_workspace(n, arr)
    if need == 0:
        raise ValueError("refit_update: ftn_refit_update_workspace rejected the counts")
    workspace = _refit_workspace("refit_update", workspace, dev, need)
    a.workspace, a.workspace_bytes = _ptr(workspace), workspace.numel()
    a.force_form = {None: 0, "one": _lib.FTN_REFIT_ONE, "grid": _lib.FTN_REFIT_GRID}[force_form]
    check(lib.ftn_refit_update(C.byref(a), _stream(dev)), "ftn_refit_update")


REFIT_LIST_MAX_TENSORS = _lib.FTN_REFIT_LIST_MAX * _lib.FTN_REFIT_MAX_TENSORS


def refit_update_list(params, grads, exp_avg, exp_avg_sq, lr: torch.Tensor, state: torch.Tensor, betas=(0.9, 0.999),
                      eps: float = 1e-8, weight_decay: float = 0.0, max_norm: Optional[float] = None, skip=(),
                      range_mask: int = 0, loss: Optional[torch.Tensor] = None, log: Optional[torch.Tensor] = None,
                      workspace: Optional[torch.Tensor] = None) -> None:
    """``ftn_refit_update_list``: ``refit_update`` for 1 to 32 tensors - consecutive groups of 8 are the records of one
    step with one global norm, one decision, one ``t`` and one log row.  Up to 8 tensors it is ``refit_update`` bit
    for bit.  ``workspace``: uint8 storage of ``ftn_refit_update_list_workspace`` bytes (None: from the caching
    allocator).  Enqueues only."""
    lib = _lib.load()
    lists = [list(params), list(grads), list(exp_avg), list(exp_avg_sq)]
    n = len(lists[0])
    if any(len(l) != n for l in lists):
        raise ValueError("refit_update_list: params, grads, exp_avg and exp_avg_sq must have one length")
    if not 1 <= n <= REFIT_LIST_MAX_TENSORS:
        raise ValueError(f"refit_update_list: {n} tensors (1..{REFIT_LIST_MAX_TENSORS} per call)")
    per = _lib.FTN_REFIT_MAX_TENSORS
    n_calls = (n + per - 1) // per
    recs = (_lib.FtnRefitArgs * n_calls)()
    counts = []
    dev = None
    for c in range(n_calls):
        sl = slice(c * per, min(n, (c + 1) * per))
        a, d, cnt = _refit_record("refit_update_list", lists[0][sl], lists[1][sl], lists[2][sl], lists[3][sl], lr,
                                  state, betas, eps, weight_decay, max_norm, skip, range_mask, loss, log)
        if dev is not None and d != dev:
            raise ValueError("refit_update_list: every tensor must be on one device")
        dev = d
        recs[c] = a
        counts.append(cnt)
    nts = (C.c_int * n_calls)(*(len(c) for c in counts))
    arrs = [(C.c_longlong * len(c))(*c) for c in counts]
    ptrs = (C.POINTER(C.c_longlong) * n_calls)(*(C.cast(a, C.POINTER(C.c_longlong)) for a in arrs))
    need = lib.ftn_refit_update_list_workspace(n_calls, nts, ptrs)
    if need == 0:
        raise ValueError("refit_update_list: ftn_refit_update_list_workspace rejected the counts")
    workspace = _refit_workspace("refit_update_list", workspace, dev, need)
    check(lib.ftn_refit_update_list(recs, n_calls, _ptr(workspace), workspace.numel(), _stream(dev)),
          "ftn_refit_update_list")


# ------------------------------------------------------------------ late-bias refit
def late_backward_form_of(B: int, Bc: int, N: int, ctx: int, S: int) -> Tuple[str, int]:
    """The kernel ``ftn_late_backward`` contracts the rows with (``ftn_late_backward_form``, host-only) and its chunks
    of series rows: ``("k_late_bwd_mfma", chunks)``.  ``Bc`` is 1 (one block of rows serves the batch) or ``B``."""
    f = _form("ftn_late_backward_form", B, Bc, N, ctx, S)
    return {_lib.FTN_LATEFIT_MFMA: "k_late_bwd_mfma"}[f & 15], f >> 4


def late_backward_workspace(B: int, Bc: int, N: int, ctx: int, S: int) -> int:
    """``ftn_late_backward_workspace``: the bytes ``late_backward`` needs (0 for a shape it does not take)."""
    return int(_lib.load().ftn_late_backward_workspace(int(B), int(Bc), int(N), int(ctx), int(S)))


def _late_operands(who: str, series_rows, gamma, beta, weight, bias, gate, rows):
    """The shapes of a late-bias call, every operand checked: ``(Bc, N, ctx, S, n_items)``.  Without ``rows`` the
    series rows are ``[Bc, N, ctx]``; with the int64 list ``rows`` ``[B]`` they are an item store ``[n_items, ctx]``
    and the call is the pipeline layout ``Bc = B``, ``N = 1``."""
    if not isinstance(series_rows, torch.Tensor) or series_rows.dim() != (3 if rows is None else 2):
        raise ValueError(f"{who} takes series rows [Bc, N, ctx]" if rows is None else
                         f"{who} takes an item store [n_items, ctx] with rows [B]")
    ctx = series_rows.shape[-1]
    if weight.dim() != 2 or weight.shape[1] != ctx:
        raise ValueError(f"{who}: weight must be [S, {ctx}], got {tuple(weight.shape)}")
    S = weight.shape[0]
    for name, t, count in (("series rows", series_rows, series_rows.numel()), ("gamma", gamma, ctx), ("beta", beta, ctx),
                           ("weight", weight, S * ctx), ("bias", bias, S), ("gate", gate, S)):
        if (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda
                or t.device != series_rows.device or not t.is_contiguous() or t.numel() != count):
            raise ValueError(f"{who}: {name} must be a contiguous fp32 device tensor of {count} elements beside the rows")
    if not 1 <= ctx <= 256 or S < 1 or series_rows.numel() < 1:
        raise ValueError(f"{who}: ctx={ctx} outside [1, 256], S={S} or no rows")
    if rows is None:
        return series_rows.shape[0], series_rows.shape[1], ctx, S, series_rows.shape[0] * series_rows.shape[1]
    return _store_rows(who, rows, series_rows).numel(), 1, ctx, S, series_rows.shape[0]


def late_fit_forward(series_rows: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, weight: torch.Tensor,
                     bias: torch.Tensor, gate: torch.Tensor, eps: float, rows=None, out=None) -> torch.Tensor:
    """``ftn_late_fit_forward``: ``late[bc, s, n] = gate[s] (weight late_bias_norm(series_rows[bc, n]) + bias)[s]``,
    ``[Bc, S, N]`` - the bits of ``context_rows``' late output for the same rows and parameters.  ``rows`` (int64
    ``[B]``): ``series_rows`` is an item store ``[n_items, ctx]``, batch row b reads item ``rows[b]`` clamped into the
    store, and the result ``[B, S, 1]`` has the bits of the plain call on ``series_rows[rows]``.  One launch."""
    lib = _lib.load()
    Bc, N, ctx, S, n_items = _late_operands("late_fit_forward", series_rows, gamma, beta, weight, bias, gate, rows)
    out = _out_or_fresh("late_fit_forward", out, (Bc, S, N), series_rows, "late")
    check(lib.ftn_late_fit_forward(_ptr(series_rows), n_items, _ptr_or_null(rows), Bc, N, ctx, S, _ptr(gamma), _ptr(beta),
                                   float(eps), _ptr(weight), _ptr(bias), _ptr(gate), _ptr(out),
                                   _stream(series_rows.device)), "ftn_late_fit_forward")
    return out


def late_backward(d_pre: torch.Tensor, series_rows: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor,
                  weight: torch.Tensor, bias: torch.Tensor, gate: torch.Tensor, eps: float, rows=None, out=None,
                  workspace: Optional[torch.Tensor] = None):
    """``ftn_late_backward``: the gradients ``(d_gamma [ctx], d_beta [ctx], d_weight [S, ctx], d_bias [S], d_gate
    [S])`` of ``late_fit_forward``'s five parameters from ``d_pre`` ``[B, S, N]``, the gradient at the rate
    pre-activation.  ``Bc == 1`` with ``B > 1``: ``d_pre`` is summed over the batch in the kernel; else ``Bc == B``.
    ``rows`` as in ``late_fit_forward`` (``d_pre`` is ``[B, S, 1]``).  ``out``: the caller's five tensors.
    ``workspace``: uint8 storage of ``late_backward_workspace`` bytes (None: from the caching allocator).  Three
    launches, enqueues only."""
    lib = _lib.load()
    who = "late_backward"
    Bc, N, ctx, S, n_items = _late_operands(who, series_rows, gamma, beta, weight, bias, gate, rows)
    if (not isinstance(d_pre, torch.Tensor) or d_pre.dim() != 3 or d_pre.dtype != torch.float32
            or d_pre.device != series_rows.device or not d_pre.is_contiguous() or tuple(d_pre.shape[1:]) != (S, N)):
        raise ValueError(f"{who}: d_pre must be contiguous fp32 [B, {S}, {N}] beside the rows")
    B = d_pre.shape[0]
    if Bc != 1 and Bc != B:
        raise ValueError(f"{who}: {Bc} row blocks for a batch of {B} (1 or the batch)")
    out = [None] * 5 if out is None else list(out)
    if len(out) != 5:
        raise ValueError(f"{who}: out is (d_gamma, d_beta, d_weight, d_bias, d_gate)")
    shapes = ((ctx,), (ctx,), (S, ctx), (S,), (S,))
    names = ("d_gamma", "d_beta", "d_weight", "d_bias", "d_gate")
    outs = [_out_or_fresh(who, o, sh, series_rows, nm) for o, sh, nm in zip(out, shapes, names)]
    need = lib.ftn_late_backward_workspace(B, Bc, N, ctx, S)
    if need == 0:
        raise ValueError(f"{who}: ftn_late_backward_workspace rejected B={B} Bc={Bc} N={N} ctx={ctx} S={S}")
    if workspace is None:
        workspace = _workspace(series_rows.device, need)
    elif (workspace.dtype != torch.uint8 or workspace.device != series_rows.device or not workspace.is_contiguous()
          or workspace.numel() < need):
        raise ValueError(f"{who}: workspace must be contiguous uint8 storage of {need} bytes beside the rows")
    check(lib.ftn_late_backward(_ptr(d_pre), B, _ptr(series_rows), n_items, _ptr_or_null(rows), Bc, N, ctx, S,
                                _ptr(gamma), _ptr(beta), float(eps), _ptr(weight), _ptr(bias), _ptr(gate),
                                *(_ptr(o) for o in outs), _ptr(workspace), workspace.numel(),
                                _stream(series_rows.device)), "ftn_late_backward")
    return tuple(outs)


# ------------------------------------------------------------------ validated refit: the end of an epoch
EPOCH_STATE_BYTES = C.sizeof(_lib.FtnEpochState)
_EPOCH_FORMS = {_lib.FTN_EPOCH_COPY_VEC: "vec", _lib.FTN_EPOCH_COPY_MIXED: "mixed"}


def refit_epoch_form_of(counts, misalign=None) -> Tuple[str, int, int]:
    """How ``ftn_refit_epoch_end`` / ``ftn_refit_epoch_restore`` copy tensors of ``counts`` elements
    (``ftn_refit_epoch_form``, host-only): ``("vec" | "mixed", scalar mask, chunks)``.  ``misalign``: per tensor the
    OR of ``address & 15`` of source and destination (None: all aligned); bit i of the mask says tensor i moves with
    scalar accesses.  More than 8 tensors or an empty one is a ValueError, as from the launch."""
    n, arr = _refit_counts(counts)
    mis = None
    if misalign is not None:
        if len(misalign) != n:
            raise ValueError(f"refit_epoch_form_of: {len(misalign)} misalign values for {n} tensors")
        mis = (C.c_int * max(n, 1))(*(int(v) for v in misalign))
    f = _lib.load().ftn_refit_epoch_form(n, arr, mis)
    if f < 0:
        check(f, "ftn_refit_epoch_form")
    return _EPOCH_FORMS[f & 15], (f >> 4) & 255, f >> 12


def _epoch_pairs(who: str, src, dst, dev):
    src, dst = list(src), list(dst)
    if len(src) != len(dst) or len(src) > _lib.FTN_EPOCH_MAX_TENSORS:
        raise ValueError(f"{who}: {len(src)} sources for {len(dst)} destinations (at most "
                         f"{_lib.FTN_EPOCH_MAX_TENSORS} pairs)")
    for s, d in zip(src, dst):
        for t in (s, d):
            if (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda or t.device != dev
                    or not t.is_contiguous() or t.numel() < 1 or t.numel() != s.numel()):
                raise ValueError(f"{who}: source and destination must be contiguous fp32 device tensors of one size "
                                 "that are not empty")
    return src, dst


def _epoch_state(who: str, state: torch.Tensor) -> None:
    if (not isinstance(state, torch.Tensor) or state.dtype != torch.uint8 or not state.is_cuda
            or not state.is_contiguous() or state.numel() != EPOCH_STATE_BYTES):
        raise ValueError(f"{who}: state must be contiguous uint8 device storage of one FtnEpochState record")


def refit_epoch_end(acc: torch.Tensor, err: torch.Tensor, den_extra: torch.Tensor, count_seen, state: torch.Tensor,
                    lr: torch.Tensor, log: torch.Tensor, patience: Optional[int] = None, plateau=None, src=(),
                    dst=()) -> None:
    """``ftn_refit_epoch_end``: the decision of a validated refit's epoch from the scorer storage ``acc`` (uint8,
    ``FtnScorePart`` records), its ``err`` word, the fp64 ``den_extra`` word and the optional int64 ``count_seen``
    word, on the ``state`` record (uint8 ``[EPOCH_STATE_BYTES]``); writes the fp32 ``lr`` word (with ``plateau``),
    one row of ``log`` (fp64 ``[max_epochs, 5]``) and zeros into the accumulators, then copies ``src[i]`` to
    ``dst[i]`` if the epoch improved.  ``patience``: None, or the epochs without improvement that are tolerated.
    ``plateau``: None or ``(factor, patience, threshold, min_lr)``.  Enqueues only."""
    who = "refit_epoch_end"
    lib = _lib.load()
    dev = state.device if isinstance(state, torch.Tensor) else None
    _epoch_state(who, state)
    if acc.dtype != torch.uint8 or acc.device != dev or not acc.is_contiguous() or acc.numel() % _lib.SCORE_PART_BYTES \
            or acc.numel() == 0:
        raise ValueError(f"{who}: acc must be contiguous uint8 device storage of FtnScorePart records")
    words = [("err", err, torch.int32), ("den_extra", den_extra, torch.float64), ("lr", lr, torch.float32)]
    if count_seen is not None:
        words.append(("count_seen", count_seen, torch.int64))
    for name, t, dtype in words:
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.numel() != 1 or t.device != dev:
            raise ValueError(f"{who}: {name} must be one {dtype} word beside the state")
    if (log.dtype != torch.float64 or log.device != dev or not log.is_contiguous() or log.dim() != 2
            or log.shape[1] != 5 or log.shape[0] < 1):
        raise ValueError(f"{who}: log must be contiguous fp64 [max_epochs >= 1, 5] beside the state")
    src, dst = _epoch_pairs(who, src, dst, dev)
    a = _lib.FtnEpochArgs()
    a.acc, a.n_slots, a.max_epochs = _ptr(acc), acc.numel() // _lib.SCORE_PART_BYTES, log.shape[0]
    a.err, a.den_extra, a.count_seen = _ptr(err), _ptr(den_extra), _ptr_or_null(count_seen)
    a.state, a.lr, a.log = _ptr(state), _ptr(lr), _ptr(log)
    a.plateau_patience, a.patience_limit = -1, -1 if patience is None else int(patience)
    if plateau is not None:
        factor, p_pat, threshold, min_lr = plateau
        a.factor, a.threshold, a.min_lr, a.plateau_patience = float(factor), float(threshold), float(min_lr), int(p_pat)
    for i, (s, d) in enumerate(zip(src, dst)):
        a.src[i], a.dst[i], a.n[i] = _ptr(s), _ptr(d), s.numel()
    a.n_tensors = len(src)
    check(lib.ftn_refit_epoch_end(C.byref(a), _stream(dev)), "ftn_refit_epoch_end")


def refit_epoch_restore(state: torch.Tensor, src, dst) -> None:
    """``ftn_refit_epoch_restore``: ``dst[i]`` gets the bits of ``src[i]`` if the ``state`` record's ``best_epoch`` is
    positive, and keeps every bit otherwise.  Enqueues only."""
    who = "refit_epoch_restore"
    _epoch_state(who, state)
    src, dst = _epoch_pairs(who, src, dst, state.device)
    n = len(src)
    if n < 1:
        raise ValueError(f"{who}: no tensors")
    ptrs = lambda ts: (C.c_void_p * n)(*(_ptr(t) for t in ts))
    _, arr = _refit_counts(t.numel() for t in src)
    check(_lib.load().ftn_refit_epoch_restore(_ptr(state), n, ptrs(src), ptrs(dst), arr, _stream(state.device)),
          "ftn_refit_epoch_restore")


# ------------------------------------------------------------------ NB CDF and quantiles
def nbq_form_of(N: int, strides=(0, 0, 0), misalign_or: int = 0) -> str:
    """The kernel form ``ftn_nb_cdf`` / ``ftn_nb_quantiles`` take (``ftn_nbq_form``, host-only: the launches dispatch
    through the same function): ``"vec4"`` (16-byte loads, four elements per lane: ``N % 4 == 0``, batch ``strides``
    of y, rate, dispersion that are multiples of 4, ``misalign_or == 0``) or ``"scalar"``."""
    f = _form("ftn_nbq_form", N, strides[0], strides[1], strides[2], misalign_or)
    return "vec4" if f & 2 else "scalar"


def nbq_form(rate, disp, y=None, out=None) -> str:
    """``nbq_form_of`` for the tensors ``nb_quantiles(rate, disp, ...)`` or, with ``y``, ``nb_cdf(y, rate, disp)`` is
    given (``out``: the output a direct ``ftn_nb_cdf`` call would pass; the wrappers' own is fresh and aligned)."""
    B, H, N = rate.shape
    ops = [t for t in (y, rate, disp, out) if t is not None]
    mis = 0
    for t in ops:
        mis |= _ptr(t) & 15
    strides = [t.stride(0) if (t is not None and B > 1) else 0 for t in (y, rate, disp)]
    return nbq_form_of(N, strides, mis)


def nb_cdf(y: torch.Tensor, rate: torch.Tensor, disp: torch.Tensor, eps: float = 1e-8, want64: bool = False,
           flag: torch.Tensor | None = None):
    """``k_nb_cdf`` over ``y``, ``rate``, ``disp`` [B,H,N] (fp32 device tensors or views with contiguous rows N
    elements apart): ``F(floor(max(y, 0)))`` as fp32 [B,H,N]; with ``want64`` returns ``(out, out64)``, the second the
    fp64 values before the rounding.  ``flag``: one device int32 that receives ``FTN_NBQ_RANGE``.  Enqueues only."""
    lib = _lib.load()
    B, H, N = _bhn_operands("nb_cdf", (("y", y), ("rate", rate), ("dispersion", disp)))
    flag = _flag_or_fresh("nb_cdf", flag, y.device, optional=True)
    out = torch.empty(B, H, N, dtype=torch.float32, device=y.device)
    out64 = torch.empty(B, H, N, dtype=torch.float64, device=y.device) if want64 else None
    check(lib.ftn_nb_cdf(_ptr(y), y.stride(0), _ptr(rate), rate.stride(0), _ptr(disp), disp.stride(0), B, H, N,
                         float(eps), _ptr(out), _ptr_or_null(out64), _ptr_or_null(flag), _stream(y.device)),
          "ftn_nb_cdf")
    return (out, out64) if want64 else out


def nb_quantiles(rate: torch.Tensor, disp: torch.Tensor, levels, eps: float = 1e-8, out: torch.Tensor | None = None,
                 flag: torch.Tensor | None = None):
    """``k_nb_quantile`` for 1..8 ``levels`` (floats strictly inside (0, 1), any order): ``out[i]`` [B,H,N] fp32 is the
    smallest integer k with ``F(k) >= levels[i]``.  ``out``: a contiguous fp32 [Q,B,H,N] to fill (default: fresh);
    ``flag``: one device int32 that receives ``FTN_NBQ_RANGE`` (default: fresh, zeroed).  Returns ``(out, flag)``.
    Enqueues only."""
    lib = _lib.load()
    B, H, N = _bhn_operands("nb_quantiles", (("rate", rate), ("dispersion", disp)))
    lv = [float(q) for q in levels]
    Q = len(lv)
    arr = (C.c_double * max(Q, 1))(*lv)
    out = _out_or_fresh("nb_quantiles", out, (Q if out is not None else max(Q, 1), B, H, N), rate)
    flag = _flag_or_fresh("nb_quantiles", flag, rate.device)
    check(lib.ftn_nb_quantiles(_ptr(rate), rate.stride(0), _ptr(disp), disp.stride(0), B, H, N, arr, Q, float(eps),
                               _ptr(out), _ptr(flag), _stream(rate.device)), "ftn_nb_quantiles")
    return out, flag


# ------------------------------------------------------------------ NB sampling
def nb_sample_form(rate, disp) -> str:
    """The kernel form ``ftn_nb_sample`` takes for these tensors (``ftn_nb_sample_form``): ``"vec4"`` or
    ``"scalar"``, by ``nbq_form_of``'s rule for rate and dispersion."""
    B, H, N = rate.shape
    f = _form("ftn_nb_sample_form", N, rate.stride(0) if B > 1 else 0, disp.stride(0) if B > 1 else 0,
              (_ptr(rate) | _ptr(disp)) & 15)
    return "vec4" if f & 2 else "scalar"


def nb_sample(rate: torch.Tensor, disp: torch.Tensor, n_samples: int = 1, seed=0, offset: int = 0, eps: float = 1e-8,
              out: torch.Tensor | None = None, flag: torch.Tensor | None = None, want_uniforms: bool = False):
    """``k_nb_sample``: ``out[s]`` [B,H,N] fp32 is draw s of the negative binomial ``(rate, disp)`` per element
    (include/flowtimes.h states the generator).  ``seed``: a Python int, or one int64 / uint64 element on the
    operands' device that the kernel reads.  ``out``: a contiguous fp32 [S,B,H,N] to fill (default: fresh); ``flag``:
    one device int32 that receives ``FTN_NBQ_RANGE`` (default: fresh, zeroed).  Returns ``(out, flag, u)``, ``u`` the
    fp64 uniforms [S,B,H,N] with ``want_uniforms``, else None.  Enqueues only."""
    lib = _lib.load()
    B, H, N = _bhn_operands("nb_sample", (("rate", rate), ("dispersion", disp)))
    S = int(n_samples)
    if S < 1:
        raise ValueError(f"nb_sample: n_samples={n_samples}")
    if not 0 <= int(offset) <= 0xFFFFFFFF:
        raise ValueError(f"nb_sample: offset={offset} is not a 32-bit word")
    seed_dev, seed_val = None, 0
    if isinstance(seed, torch.Tensor):
        if (seed.numel() != 1 or seed.dtype not in (torch.int64, torch.uint64) or seed.device != rate.device):
            raise ValueError("nb_sample: a seed tensor must be one int64 / uint64 element on the operands' device")
        seed_dev = seed
    else:
        seed_val = int(seed) & 0xFFFFFFFFFFFFFFFF
    out = _out_or_fresh("nb_sample", out, (S, B, H, N), rate)
    u = torch.empty(S, B, H, N, dtype=torch.float64, device=rate.device) if want_uniforms else None
    flag = _flag_or_fresh("nb_sample", flag, rate.device)
    check(lib.ftn_nb_sample(_ptr(rate), rate.stride(0), _ptr(disp), disp.stride(0), B, H, N, S, seed_val,
                            _ptr_or_null(seed_dev), int(offset), float(eps), _ptr(out), _ptr_or_null(u), _ptr(flag),
                            _stream(rate.device)), "ftn_nb_sample")
    return out, flag, u


# ------------------------------------------------------------------ path summaries
PATH_REDUCE = {"sum": _lib.FTN_PATH_SUM, "max": _lib.FTN_PATH_MAX}


def path_summary_form_of(P: int, N: int, window: int = 1, strides=(0, 0, 0), misalign_or: int = 0) -> str:
    """The kernel form ``ftn_path_summary`` takes (``ftn_path_summary_form``, host-only: the launch dispatches through
    the same function): ``"reg<PP>/vec4"``, ``"reg<PP>/scalar"`` (a lane sorts its columns in registers, PP the
    padded P) or ``"lds<PP>x<T>/vec4"``, ``"lds<PP>x<T>/scalar"`` (a workgroup sorts a tile of T columns in LDS).
    ``strides``: the path and batch strides of samples and the batch stride of y, in elements."""
    f = _form("ftn_path_summary_form", P, N, window, strides[0], strides[1], strides[2], misalign_or)
    width = "vec4" if f & 2 else "scalar"
    pp = (f >> 8) & 0xFFF
    return f"lds{pp}x{f >> 20}/{width}" if f & _lib.FTN_PATH_LDS else f"reg{pp}/{width}"


def _path_strides(samples, y):
    P, B, H, N = samples.shape
    return (samples.stride(0) if P > 1 else 0, samples.stride(1) if B > 1 else 0,
            y.stride(0) if (y is not None and B > 1) else 0)


def path_summary_form(samples, y=None, window: int = 1, outs=()) -> str:
    """``path_summary_form_of`` for the tensors ``path_summary(samples, ..., y=y)`` is given (``outs``: outputs a
    direct call would pass; the wrapper's own are fresh and aligned)."""
    mis = 0
    for t in (samples, y, *outs):
        if t is not None:
            mis |= _ptr(t) & 15
    return path_summary_form_of(samples.shape[0], samples.shape[3], window, _path_strides(samples, y), mis)


def _path_operands(samples, y) -> None:
    """Shape, then row layout, then dtype and device of samples [P,B,H,N] and y [B,H,N], as ``_bhn_operands``."""
    if not isinstance(samples, torch.Tensor) or samples.dim() != 4:
        raise ValueError("path_summary: samples must be a [P, B, H, N] tensor")
    P, B, H, N = samples.shape
    if P < 1 or B < 1 or H < 1 or N < 1:
        raise ValueError(f"path_summary: empty shape {tuple(samples.shape)}")
    if y is not None and (not isinstance(y, torch.Tensor) or tuple(y.shape) != (B, H, N)):
        raise ValueError(f"path_summary: y must be a {(B, H, N)} tensor beside samples {tuple(samples.shape)}")
    if not rows_ok(samples):
        raise ValueError(f"path_summary: samples need contiguous rows N elements apart, strides {samples.stride()}")
    if y is not None and not rows_ok(y):
        raise ValueError(f"path_summary: y needs contiguous rows N elements apart, strides {y.stride()}")
    for name, t in (("samples", samples), ("y", y)):
        if t is not None and (t.dtype != torch.float32 or not t.is_cuda or t.device != samples.device):
            raise ValueError(f"path_summary: {name} must be an fp32 tensor on samples' device, got {t.dtype} on "
                             f"{t.device}")


def path_summary(samples: torch.Tensor, ranks, window: int = 1, reduce: str = "sum", y: torch.Tensor | None = None,
                 want_mean: bool = True, want_sorted: bool = False, out: dict | None = None):
    """``ftn_path_summary`` over ``samples`` [P,B,H,N] (an fp32 device tensor or a view with contiguous rows N
    elements apart): per element of [B,H',N], ``H' = H / window``, of the window sums or maxima of every path, the
    order statistics at ``ranks`` (ints in 1..P, any number: one launch per 8), the mean, the sample CRPS against
    ``y`` [B,H,N] when it is given, and the sorted column with ``want_sorted``.  Mean, CRPS and sorted column come
    from the first launch.  ``out``: contiguous fp32 tensors to fill under the keys of the result (default: fresh).
    Returns ``{"quantiles": [Q,B,H',N], "mean": .., "crps": .., "sorted": [P,B,H',N]}`` with None for what was not
    asked for.  Enqueues only."""
    lib = _lib.load()
    _path_operands(samples, y)
    if reduce not in PATH_REDUCE:
        raise ValueError(f"path_summary: reduce {reduce!r} is not 'sum' or 'max'")
    P, B, H, N = samples.shape
    w = int(window)
    if w < 1 or H % w:
        raise ValueError(f"path_summary: window={window} does not divide H={H}")
    Hp = H // w
    rk = [int(r) for r in ranks]
    for r in rk:
        if not 1 <= r <= P:
            raise ValueError(f"path_summary: rank {r} is outside 1..{P}")
    Q = len(rk)
    shapes = {"quantiles": (Q, B, Hp, N) if Q else None, "mean": (B, Hp, N) if want_mean else None,
              "crps": (B, Hp, N) if y is not None else None, "sorted": (P, B, Hp, N) if want_sorted else None}
    res = {}
    for key, shape in shapes.items():
        given = None if out is None else out.get(key)
        res[key] = None if shape is None else _out_or_fresh("path_summary", given, shape, samples, f"out[{key!r}]")
    ps, bs, ybs = samples.stride(0), samples.stride(1), (y.stride(0) if y is not None else 0)
    first = True
    for i in range(0, max(Q, 1), _lib.FTN_QMAX):
        part = rk[i:i + _lib.FTN_QMAX]
        arr = (C.c_int * max(len(part), 1))(*part)
        q_out = res["quantiles"][i:i + len(part)] if part else None
        check(lib.ftn_path_summary(_ptr(samples), ps, bs, P, B, H, N, w, PATH_REDUCE[reduce],
                                   _ptr_or_null(y if first else None), ybs, arr, len(part), _ptr_or_null(q_out),
                                   _ptr_or_null(res["mean"] if first else None),
                                   _ptr_or_null(res["crps"] if first else None),
                                   _ptr_or_null(res["sorted"] if first else None), _stream(samples.device)),
              "ftn_path_summary")
        first = False
    return res


# ------------------------------------------------------------------ series groups
def group_sum_form_of(N: int, row_stride: int | None = None, misalign_or: int = 0, n_chunks: int = 0) -> str:
    """The kernel form ``ftn_group_sum`` takes (``ftn_group_sum_form``, host-only: the launch dispatches through the
    same function): ``"vec4/t<T>"`` or ``"scalar/t<T>"``, the load width of x and the rows of a tile.  ``row_stride``
    in elements (default: N), ``misalign_or`` the address of x modulo 16, ``n_chunks`` the chunks of 32 members over
    all groups."""
    f = _form("ftn_group_sum_form", N, N if row_stride is None else row_stride, misalign_or, n_chunks)
    return f"{'vec4' if f & 2 else 'scalar'}/t{f >> 8}"


def _csr_chunks(offsets_host) -> int:
    """The chunks of 32 members over all groups of the CSR offsets."""
    sizes = [int(b) - int(a) for a, b in zip(offsets_host[:-1], offsets_host[1:])]
    return sum((m + _lib.FTN_GROUP_CHUNK - 1) // _lib.FTN_GROUP_CHUNK for m in sizes)


def _group_csr(who: str, x: torch.Tensor, order, offsets, offsets_host) -> Tuple[int, int]:
    """``(G, M)`` of the CSR ``order`` [M] / ``offsets`` [G+1] / ``offsets_host`` for ``x``, fp32 on a ROCm device."""
    xn = "x3" if x.dim() == 3 else "x"
    if x.dtype != torch.float32 or not x.is_cuda:
        raise ValueError(f"{who}: {xn} must be an fp32 tensor on a ROCm device, got {x.dtype} on {x.device}")
    for name, t in (("order", order), ("offsets", offsets)):
        if (not isinstance(t, torch.Tensor) or t.dim() != 1 or t.dtype != torch.int32 or t.device != x.device
                or not t.is_contiguous()):
            raise ValueError(f"{who}: {name} must be a contiguous int32 vector on {xn}'s device")
    G, M = offsets.numel() - 1, order.numel()
    if (getattr(offsets_host, "dtype", None) != "int32" or offsets_host.ndim != 1 or offsets_host.size != G + 1
            or not offsets_host.flags["C_CONTIGUOUS"]):
        raise ValueError(f"{who}: offsets_host must be a contiguous int32 numpy array of {G + 1} offsets")
    return G, M


def group_sum_form(x: torch.Tensor, offsets_host) -> str:
    """``group_sum_form_of`` for the tensors ``group_sum(x, order, offsets, offsets_host)`` is given."""
    rows, N = x.shape
    return group_sum_form_of(N, x.stride(0) if rows > 1 else N, _ptr(x) & 15, _csr_chunks(offsets_host))


def group_sum(x: torch.Tensor, order: torch.Tensor, offsets: torch.Tensor, offsets_host, out: torch.Tensor | None = None
              ) -> torch.Tensor:
    """``ftn_group_sum``: ``x`` [rows, N] fp32 on a ROCm device, elements contiguous and rows ``x.stride(0) >= N``
    apart; ``order`` [M] and ``offsets`` [G+1] the int32 CSR member lists on that device, ``offsets_host`` the same
    G+1 offsets as a contiguous int32 numpy array.  Returns ``out`` [rows, G] fp32 (default: fresh; else a contiguous
    one to fill).  Enqueues only."""
    lib = _lib.load()
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.numel() == 0:
        raise ValueError("group_sum: x must be a non-empty [rows, N] tensor")
    rows, N = x.shape
    if (N > 1 and x.stride(1) != 1) or (rows > 1 and x.stride(0) < N):
        raise ValueError(f"group_sum: x needs contiguous rows at least N apart, strides {x.stride()}")
    G, M = _group_csr("group_sum", x, order, offsets, offsets_host)
    out = _out_or_fresh("group_sum", out, (rows, G), x)
    check(lib.ftn_group_sum(_ptr(x), rows, N, x.stride(0) if rows > 1 else N, _ptr(order) if M else None,
                            _ptr(offsets), offsets_host.ctypes.data, G, M, _ptr(out), _stream(x.device)),
          "ftn_group_sum")
    return out


def group_sum_rows_form_of(inner: int, member_stride: int | None = None, outer_stride: int = 0, misalign_or: int = 0,
                           n_chunks: int = 0) -> str:
    """The kernel form ``ftn_group_sum_rows`` takes (``ftn_group_sum_rows_form``, host-only: the launch dispatches
    through the same function): ``"vec4/i<TI>"`` or ``"scalar/i<TI>"``, the load and store width along ``inner`` and
    the inner columns of a tile (bits 16-27 of the word, the passes a tile takes over the chunks, are not part of the
    name).  Strides in elements (``member_stride`` default: ``inner``; ``outer_stride`` 0 for
    one slab), ``misalign_or`` the addresses of x and out, or-ed, modulo 16, ``n_chunks`` the chunks of 32 members
    over all groups."""
    f = _form("ftn_group_sum_rows_form", inner, inner if member_stride is None else member_stride, outer_stride,
              misalign_or, n_chunks)
    return f"{'vec4' if f & 2 else 'scalar'}/i{(f >> 8) & 255}"


def _rows_strides(x3: torch.Tensor) -> Tuple[int, int]:
    """``(outer_stride, member_stride)`` as ``ftn_group_sum_rows`` takes them: a stride that addresses nothing (one
    slab, one member) is replaced by the dense one."""
    outer, S, inner = x3.shape
    ms = x3.stride(1) if S > 1 else inner
    return (x3.stride(0) if outer > 1 else 0), ms


def group_sum_rows_form(x3: torch.Tensor, offsets_host, out: torch.Tensor | None = None) -> str:
    """``group_sum_rows_form_of`` for the tensors ``group_sum_rows(x3, order, offsets, offsets_host, out)`` is given
    (a fresh ``out`` is 16-byte aligned)."""
    os_, ms = _rows_strides(x3)
    mis = (_ptr(x3) | (0 if out is None else _ptr(out))) & 15
    return group_sum_rows_form_of(x3.shape[2], ms, os_, mis, _csr_chunks(offsets_host))


def group_sum_rows(x3: torch.Tensor, order: torch.Tensor, offsets: torch.Tensor, offsets_host,
                   out: torch.Tensor | None = None) -> torch.Tensor:
    """``ftn_group_sum_rows``: ``x3`` [outer, S, inner] fp32 on a ROCm device, ``inner`` contiguous
    (``x3.stride(2) == 1``), members ``x3.stride(1) >= inner`` apart and slabs ``x3.stride(0) >= S x3.stride(1)``
    apart; the groups are over the S members of dim 1: ``order`` [M] and ``offsets`` [G+1] the int32 CSR member lists
    on that device, ``offsets_host`` the same G+1 offsets as a contiguous int32 numpy array.  Returns ``out``
    [outer, G, inner] fp32 (default: fresh; else a contiguous one to fill).  Enqueues only."""
    lib = _lib.load()
    if not isinstance(x3, torch.Tensor) or x3.dim() != 3 or x3.numel() == 0:
        raise ValueError("group_sum_rows: x3 must be a non-empty [outer, S, inner] tensor")
    outer, S, inner = x3.shape
    if ((inner > 1 and x3.stride(2) != 1) or (S > 1 and x3.stride(1) < inner)
            or (outer > 1 and x3.stride(0) < S * (x3.stride(1) if S > 1 else inner))):
        raise ValueError(f"group_sum_rows: x3 needs contiguous inner elements, members at least inner apart and slabs "
                         f"at least S members apart, strides {x3.stride()}")
    G, M = _group_csr("group_sum_rows", x3, order, offsets, offsets_host)
    out = _out_or_fresh("group_sum_rows", out, (outer, G, inner), x3)
    os_, ms = _rows_strides(x3)
    check(lib.ftn_group_sum_rows(_ptr(x3), outer, S, inner, os_, ms, _ptr(order) if M else None, _ptr(offsets),
                                 offsets_host.ctypes.data, G, M, _ptr(out), _stream(x3.device)),
          "ftn_group_sum_rows")
    return out


# ------------------------------------------------------------------ device windows
WINDOW_LAYOUTS = {"series": _lib.FTN_WIN_SERIES, "wide": _lib.FTN_WIN_WIDE}
WINDOW_PIECES = ("x", "y", "mask", "x_mark", "y_mark", "static", "id")
_WINDOW_FIELD = {"static": "static_out", "id": "id_out"}


def _window_layout(who: str, layout) -> int:
    if layout not in WINDOW_LAYOUTS:
        raise ValueError(f"{who}: layout {layout!r} is not 'series' or 'wide'")
    return WINDOW_LAYOUTS[layout]


def _window_form_word(a: "_lib.FtnWindowArgs") -> dict:
    f = _lib.load().ftn_window_batch_form(C.byref(a))
    if f < 0:
        check(f, "ftn_window_batch_form")
    tile = ((f >> 8) & 255, (f >> 16) & 255)
    return {"vec": tuple(n for b, n in enumerate(WINDOW_PIECES[:5]) if f >> b & 1), "tile": tile if tile[0] else None}


def window_batch_form_of(layout: str, N: int, L: int, H: int, F: int = 0, Fs: int = 0, outs=("x", "y", "mask"),
                         x_stride: int | None = None, m_stride: int | None = None, marks_stride: int | None = None,
                         has_mask: bool = True, misalign: dict | None = None) -> dict:
    """The kernel form ``ftn_window_batch`` takes (``ftn_window_batch_form``, host-only: the launch dispatches through
    the same function) for the outputs named in ``outs``: ``{"vec": the pieces among x, y, mask, x_mark, y_mark that
    move 16 bytes a lane, "tile": (series, steps) of the transposition or None}``.  Row strides in elements (default:
    dense), ``has_mask`` whether a validity table is given, ``misalign`` the byte offsets from a 16-byte boundary of
    the tables ``"X"``, ``"M"``, ``"marks"`` and of the outputs by name (default 0)."""
    mis = dict(misalign or {})
    a = _lib.FtnWindowArgs()
    a.layout = _window_layout("window_batch_form_of", layout)
    a.N, a.L, a.H, a.F, a.Fs = int(N), int(L), int(H), int(F), int(Fs)
    a.x_stride = int(N if x_stride is None else x_stride)
    a.m_stride = int(N if m_stride is None else m_stride)
    a.marks_stride = int(F if marks_stride is None else marks_stride)
    a.X = 0x100000 + mis.pop("X", 0)                            # stand-in addresses: the form reads their low bits only
    a.M = 0x200000 + mis.pop("M", 0) if has_mask else None
    a.marks = 0x300000 + mis.pop("marks", 0) if F else None
    a.statics = 0x400000 if Fs else None
    a.ids = 0x500000 if "id" in outs else None
    for at, name in enumerate(outs):
        if name not in WINDOW_PIECES:
            raise ValueError(f"window_batch_form_of: {name!r} is not one of {WINDOW_PIECES}")
        setattr(a, _WINDOW_FIELD.get(name, name), 0x1000000 * (at + 1) + mis.pop(name, 0))
    if mis:
        raise ValueError(f"window_batch_form_of: misalign names {sorted(mis)} are neither tables nor requested outputs")
    return _window_form_word(a)


def _window_table(who: str, name: str, t, cols: int | None, like: torch.Tensor | None, dtype=torch.float32):
    """``(pointer, row stride, rows, columns)`` of an optional 2-D table with contiguous elements."""
    if t is None:
        return None, 0, 0, 0
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.numel() == 0:
        raise ValueError(f"{who}: {name} must be a non-empty 2-D tensor")
    if t.dtype != dtype or not t.is_cuda or (like is not None and t.device != like.device):
        raise ValueError(f"{who}: {name} must be {dtype} on {'a ROCm device' if like is None else like.device}, got "
                         f"{t.dtype} on {t.device}")
    rows, c = t.shape
    if cols is not None and c != cols:
        raise ValueError(f"{who}: {name} has {c} columns, not {cols}")
    if (c > 1 and t.stride(1) != 1) or (rows > 1 and t.stride(0) < c):
        raise ValueError(f"{who}: {name} needs contiguous rows at least {c} apart, strides {t.stride()}")
    return _ptr(t), (t.stride(0) if rows > 1 else c), rows, c


def _window_args(who: str, X, L, H, M, marks, statics, ids, layout, outs: dict, count: int | None):
    a = _lib.FtnWindowArgs()
    a.layout = _window_layout(who, layout)
    a.X, a.x_stride, T, N = _window_table(who, "X", X, None, None)
    if X is None:
        raise ValueError(f"{who}: X is required")
    a.M, a.m_stride, Tm, _ = _window_table(who, "M", M, N, X)
    a.marks, a.marks_stride, Tk, F = _window_table(who, "marks", marks, None, X)
    if (M is not None and Tm != T) or (marks is not None and Tk != T):
        raise ValueError(f"{who}: M and marks must have X's {T} rows")
    for name, t in (("statics", statics), ("ids", ids)):
        if t is not None and (not isinstance(t, torch.Tensor) or not t.is_contiguous() or t.device != X.device
                              or t.shape[0] != N or t.dim() != (2 if name == "statics" else 1)
                              or t.dtype != (torch.float32 if name == "statics" else torch.int64)):
            raise ValueError(f"{who}: {name} must be a contiguous {'fp32 [N, Fs]' if name == 'statics' else 'int64 [N]'} "
                             f"tensor beside X")
    Fs = statics.shape[1] if statics is not None else 0
    a.statics, a.ids = _ptr_or_null(statics), _ptr_or_null(ids)
    a.T, a.N, a.L, a.H, a.F, a.Fs = T, N, int(L), int(H), F, Fs
    wide = layout == "wide"
    per_item = {"x": int(L) * (N if wide else 1), "y": int(H) * (N if wide else 1), "mask": int(H) * (N if wide else 1),
                "x_mark": int(L) * F, "y_mark": int(H) * F, "static": Fs, "id": 1}
    for name, t in outs.items():
        if name not in WINDOW_PIECES:
            raise ValueError(f"{who}: output {name!r} is not one of {WINDOW_PIECES}")
        if t is None:
            continue
        want = torch.int64 if name == "id" else torch.float32
        if (not isinstance(t, torch.Tensor) or t.dtype != want or t.device != X.device or not t.is_contiguous()
                or (count is not None and (t.dim() < 1 or t.shape[0] != count or t.numel() != count * per_item[name]))):
            raise ValueError(f"{who}: output {name!r} must be a contiguous {want} tensor beside X with {count} rows of "
                             f"{per_item[name]} elements, got {tuple(getattr(t, 'shape', ()))}")
        setattr(a, _WINDOW_FIELD.get(name, name), _ptr(t))
    return a


def window_batch_form(X: torch.Tensor, L: int, H: int, outs: dict, M=None, marks=None, statics=None, ids=None,
                      layout: str = "series") -> dict:
    """``window_batch_form_of`` for the tensors ``window_batch`` is given: ``outs`` maps piece names to the output
    tensors (their addresses enter the form)."""
    return _window_form_word(_window_args("window_batch_form", X, L, H, M, marks, statics, ids, layout, outs, None))


def window_batch(X: torch.Tensor, starts: torch.Tensor, starts_host, L: int, H: int, item0: int, count: int,
                 outs: dict, M=None, marks=None, statics=None, ids=None, layout: str = "series") -> None:
    """``ftn_window_batch``: fills rows ``0 .. count - 1`` of the tensors in ``outs`` (piece name -> contiguous tensor
    whose first dim is ``count``: ``x``, ``y``, ``mask``, ``x_mark``, ``y_mark``, ``static`` fp32, ``id`` int64) with
    items ``item0 .. item0 + count - 1`` of the tables ``X`` [T, N], ``M`` [T, N], ``marks`` [T, F] (fp32, elements
    contiguous, rows at least a row apart: row and column slices are fine), ``statics`` [N, Fs] and ``ids`` [N] int64,
    all on one ROCm device.  ``starts`` [W] int32 on that device are the window start rows, ``starts_host`` the same
    words as a contiguous int32 numpy array.  One launch on the current stream; enqueues only."""
    who = "window_batch"
    a = _window_args(who, X, L, H, M, marks, statics, ids, layout, outs, int(count))
    _window_starts(who, a, X, starts, starts_host)
    a.item0, a.count = int(item0), int(count)
    check(_lib.load().ftn_window_batch(C.byref(a), _stream(X.device)), "ftn_window_batch")


def _window_starts(who: str, a, X, starts, starts_host) -> None:
    if (not isinstance(starts, torch.Tensor) or starts.dim() != 1 or starts.dtype != torch.int32
            or starts.device != X.device or not starts.is_contiguous()):
        raise ValueError(f"{who}: starts must be a contiguous int32 vector on X's device")
    W = starts.numel()
    if (getattr(starts_host, "dtype", None) != "int32" or starts_host.ndim != 1 or starts_host.size != W
            or not starts_host.flags["C_CONTIGUOUS"]):
        raise ValueError(f"{who}: starts_host must be a contiguous int32 numpy array of {W} start rows")
    a.starts, a.starts_host, a.W = _ptr(starts), starts_host.ctypes.data, W


# ------------------------------------------------------------------ training windows
WINDOW_EPOCH_MAX = 1 << 30


def window_epoch_check(who: str, seed, epoch, ts=0, noise_std=0.0):
    """``(seed, epoch, ts, noise_std)`` as the words the generator takes, or a ValueError: ``seed`` is taken modulo
    2^64, ``0 <= epoch < 2^30``, ``ts >= 0`` with ``2 ts + 1 < 2^32`` (and within the int32 the C entry takes),
    ``noise_std`` finite and not negative."""
    epoch, ts, sd = int(epoch), int(ts), float(noise_std)
    if not 0 <= epoch < WINDOW_EPOCH_MAX:
        raise ValueError(f"{who}: epoch={epoch} is outside [0, 2^30)")
    if ts < 0 or 2 * ts + 1 >= 1 << 32:
        raise ValueError(f"{who}: time_shift={ts} must be >= 0 with 2 time_shift + 1 < 2^32")
    if not 0.0 <= sd < float("inf"):
        raise ValueError(f"{who}: add_noise_std={noise_std} must be finite and >= 0")
    return int(seed) & 0xFFFFFFFFFFFFFFFF, epoch, ts, sd


def epoch_keys(n: int, seed: int, epoch: int, device) -> torch.Tensor:
    """``ftn_epoch_keys``: int64 ``[n]`` on ``device`` (a ROCm device), ``key64(k)`` of the epoch's order for
    ``k < n``; the order is ``torch.argsort(keys, stable=True)``.  One launch on the current stream."""
    who = "epoch_keys"
    seed, epoch, _, _ = window_epoch_check(who, seed, epoch)
    device = torch.device(device)
    if int(n) < 1 or device.type != "cuda":
        raise ValueError(f"{who}: n={n} keys on {device}: n must be positive and the device a ROCm device")
    keys = torch.empty(int(n), dtype=torch.int64, device=device)
    check(_lib.load().ftn_epoch_keys(int(n), seed, epoch, _ptr(keys), _stream(keys.device)), "ftn_epoch_keys")
    return keys


def window_gather(X: torch.Tensor, starts: torch.Tensor, starts_host, L: int, H: int, item_lo: int,
                  items: torch.Tensor, outs: dict, XT=None, M=None, MT=None, marks=None, statics=None, ids=None,
                  layout: str = "series", time_shift: int = 0, noise_std: float = 0.0, seed: int = 0,
                  epoch: int = 0) -> None:
    """``ftn_window_gather``: fills rows ``0 .. count - 1`` of the tensors in ``outs`` (as for ``window_batch``) with
    the items ``items`` (contiguous int64 ``[count]`` on X's device, global indices, not read back) that belong to
    this part, whose first item is ``item_lo``; the other rows are left untouched.  ``XT`` [N, T] (and ``MT``) are the
    series-major copies the series layout reads (rows contiguous, at least T apart); the wide layout reads ``X`` and
    ``M``.  ``time_shift``, ``noise_std``, ``seed`` and ``epoch`` as in include/flowtimes.h.  One launch on the
    current stream; enqueues only."""
    who = "window_gather"
    seed, epoch, ts, sd = window_epoch_check(who, seed, epoch, time_shift, noise_std)
    if (not isinstance(items, torch.Tensor) or items.dim() != 1 or items.dtype != torch.int64 or items.numel() < 1
            or not items.is_contiguous() or not isinstance(X, torch.Tensor) or items.device != X.device):
        raise ValueError(f"{who}: items must be a non-empty contiguous int64 vector on X's device")
    count = items.numel()
    g = _lib.FtnWindowGatherArgs()
    g.w = _window_args(who, X, L, H, M, marks, statics, ids, layout, outs, count)
    a = g.w                                                     # a view of the embedded record
    _window_starts(who, a, X, starts, starts_host)
    if int(item_lo) < 0:
        raise ValueError(f"{who}: item_lo={item_lo} is negative")
    a.item0, a.count = int(item_lo), count
    if layout == "series":
        if XT is None:
            raise ValueError(f"{who}: the series layout takes XT, the series-major copy of X")
        g.XT, g.xt_stride, Nx, Tx = _window_table(who, "XT", XT, None, X)
        g.MT, g.mt_stride, Nm, Tm = _window_table(who, "MT", MT, None, X)
        if (Nx, Tx) != (a.N, a.T) or (MT is not None and (Nm, Tm) != (a.N, a.T)) or (M is None) != (MT is None):
            raise ValueError(f"{who}: XT (and MT beside M) must be [N, T] = [{a.N}, {a.T}]")
    g.items, g.seed, g.noise_std, g.epoch, g.ts = _ptr(items), seed, sd, epoch, ts
    check(_lib.load().ftn_window_gather(C.byref(g), _stream(X.device)), "ftn_window_gather")


# ------------------------------------------------------------------ table preparation
TABLE_METHODS = {"zscore": _lib.FTN_TAB_ZSCORE, "minmax": _lib.FTN_TAB_MINMAX}
_TABLE_FORM_FIELDS = ("load_bytes", "col_tile", "block", "chunk", "resident", "partials", "lane_axis")


def _table_form(name: str, args) -> dict:
    f = _lib.FtnTableForm()
    rc = getattr(_lib.load(), name)(C.byref(args), C.byref(f))
    if rc < 0:
        check(rc, name)
    return {k: getattr(f, k) for k in _TABLE_FORM_FIELDS}


def _table_flags(clip: bool, mask: bool, diffs: bool) -> int:
    return (_lib.FTN_TAB_CLIP if clip else 0) | (_lib.FTN_TAB_MASK if mask else 0) | (_lib.FTN_TAB_DIFF if diffs else 0)


def table_moments_form_of(T: int, N: int, x_stride: int | None = None, m_stride: int | None = None,
                          mask: bool = False, diffs: bool = False, clip: bool = False,
                          misalign: dict | None = None) -> dict:
    """The form ``ftn_table_moments`` takes (``ftn_table_moments_form``, host-only: the launch dispatches through the
    same function): ``load_bytes`` 16 or 4, ``col_tile`` columns a workgroup, ``block`` rows a row block, ``partials``
    row blocks.  Row strides in elements (default: dense); ``misalign``: byte offsets of ``"X"`` / ``"M"`` from a
    16-byte boundary."""
    mis = dict(misalign or {})
    a = _lib.FtnTableMomentsArgs()
    a.T, a.N, a.flags = int(T), int(N), _table_flags(clip, mask, diffs)
    a.x_stride = int(N if x_stride is None else x_stride)
    a.m_stride = int(N if m_stride is None else m_stride)
    a.X = 0x100000 + mis.pop("X", 0)                            # stand-in addresses: the form reads their low bits only
    m_off = mis.pop("M", 0)
    a.M = 0x200000 + m_off if mask else None
    if mis:
        raise ValueError(f"table_moments_form_of: misalign names {sorted(mis)} are not tables of the call")
    return _table_form("ftn_table_moments_form", a)


def _table_pair(who: str, X, M):
    """The pointers and row strides of a table ``X`` [T, N] and its optional validity ``M``."""
    xp, xs, T, N = _window_table(who, "X", X, None, None)
    if X is None:
        raise ValueError(f"{who}: X is required")
    mp, ms, Tm, _ = _window_table(who, "M", M, N, X)
    if M is not None and Tm != T:
        raise ValueError(f"{who}: M must have X's {T} rows")
    return xp, xs, mp, ms, T, N


def table_moments(X: torch.Tensor, M: torch.Tensor | None = None, clip: bool = False, diffs: bool = False,
                  form: bool = False, out: torch.Tensor | None = None):
    """``ftn_table_moments``: the column statistics fp64 ``[6, N]`` (count, sum, mean, centred sum of squares, min,
    max; ``[12, N]`` with ``diffs``: the same of the first differences) of the fp32 device table ``X`` [T, N]
    (elements contiguous, rows at least a row apart); ``M`` given: only elements with ``M > 0`` count.  Enqueues
    four launches on the current stream.  ``out``: the contiguous fp64 statistics tensor to fill.  ``form=True``: the
    form dict of this call instead."""
    who = "table_moments"
    a = _lib.FtnTableMomentsArgs()
    a.X, a.x_stride, a.M, a.m_stride, a.T, a.N = _table_pair(who, X, M)
    a.flags = _table_flags(clip, M is not None, diffs)
    if form:
        return _table_form("ftn_table_moments_form", a)
    lib = _lib.load()
    rows = 12 if diffs else 6
    stats = torch.empty(rows, a.N, dtype=torch.float64, device=X.device) if out is None else out
    if stats.shape != (rows, a.N) or stats.dtype != torch.float64 or stats.device != X.device or not stats.is_contiguous():
        raise ValueError(f"{who}: out must be a contiguous fp64 [{rows}, {a.N}] tensor beside X")
    nbytes = int(lib.ftn_table_moments_bytes(a.T, a.N))
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=X.device)
    a.stats, a.workspace, a.workspace_bytes = _ptr(stats), _ptr(ws), nbytes
    check(lib.ftn_table_moments(C.byref(a), _stream(X.device)), "ftn_table_moments")
    return stats


def table_spectrum_form_of(T: int, N: int, x_stride: int | None = None, m_stride: int | None = None,
                           has_mask: bool = True, misalign: dict | None = None) -> dict:
    """The form ``ftn_table_spectrum`` takes (``ftn_table_spectrum_form``, host-only): ``load_bytes`` of the staging
    loads, ``col_tile`` columns and ``block`` bins a workgroup, ``chunk`` rows a staging chunk, ``resident`` whether
    the column tile is one chunk, ``partials`` bin blocks."""
    mis = dict(misalign or {})
    a = _lib.FtnTableSpectrumArgs()
    a.T, a.N = int(T), int(N)
    a.x_stride = int(N if x_stride is None else x_stride)
    a.m_stride = int(N if m_stride is None else m_stride)
    a.X = 0x100000 + mis.pop("X", 0)
    m_off = mis.pop("M", 0)
    a.M = 0x200000 + m_off if has_mask else None
    if mis:
        raise ValueError(f"table_spectrum_form_of: misalign names {sorted(mis)} are not tables of the call")
    return _table_form("ftn_table_spectrum_form", a)


def table_spectrum(X: torch.Tensor, mean: torch.Tensor, M: torch.Tensor | None = None, power_out=None,
                   form: bool = False, outs=None):
    """``ftn_table_spectrum``: per column of the fp32 device table ``X`` [T, N], demeaned by ``mean`` [N] fp32 and
    masked by ``M > 0``: ``(f_peak int32 [N], peak fp32 [N], total fp32 [N])`` of the power at bins 1 .. T // 2.
    ``power_out``: a contiguous fp32 ``[T // 2, N]`` tensor that receives every bin (tests).  ``outs``: the three
    output tensors to fill.  Two launches on the current stream; the twiddle table is cached per ``T``."""
    who = "table_spectrum"
    a = _lib.FtnTableSpectrumArgs()
    a.X, a.x_stride, a.M, a.m_stride, a.T, a.N = _table_pair(who, X, M)
    if form:
        return _table_form("ftn_table_spectrum_form", a)
    T, N, dev = a.T, a.N, X.device
    if not isinstance(mean, torch.Tensor) or mean.shape != (N,) or mean.dtype != torch.float32 or mean.device != dev \
            or not mean.is_contiguous():
        raise ValueError(f"{who}: mean must be a contiguous fp32 [N] = [{N}] tensor beside X")
    lib = _lib.load()
    if outs is None:
        outs = (torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.float32, device=dev),
                torch.empty(N, dtype=torch.float32, device=dev))
    f_peak, peak, total = outs
    for t, dt in ((f_peak, torch.int32), (peak, torch.float32), (total, torch.float32)):
        if t.shape != (N,) or t.dtype != dt or t.device != dev or not t.is_contiguous():
            raise ValueError(f"{who}: outs must be contiguous [N] tensors (int32, fp32, fp32) beside X")
    if power_out is not None and (power_out.shape != (T // 2, N) or power_out.dtype != torch.float32
                                  or power_out.device != dev or not power_out.is_contiguous()):
        raise ValueError(f"{who}: power_out must be a contiguous fp32 [T // 2, N] = [{T // 2}, {N}] tensor beside X")
    tw = state(dev).table_twiddles(T)
    nbytes = int(lib.ftn_table_spectrum_bytes(T, N))
    ws = torch.empty(max(nbytes, 8) // 8, dtype=torch.float64, device=dev)
    a.mean, a.twiddle = _ptr(mean), _ptr(tw)
    a.f_peak, a.peak, a.total = _ptr(f_peak), _ptr(peak), _ptr(total)
    a.power_out = _ptr(power_out) if power_out is not None and power_out.numel() else None
    a.workspace, a.workspace_bytes = _ptr(ws), nbytes
    check(lib.ftn_table_spectrum(C.byref(a), _stream(dev)), "ftn_table_spectrum")
    return f_peak, peak, total


def table_features(stats: torch.Tensor, f_peak: torch.Tensor, peak: torch.Tensor, total: torch.Tensor, T: int,
                   out: torch.Tensor | None = None) -> torch.Tensor:
    """``ftn_table_features``: the five features fp32 ``[N, 5]`` from the ``[12, N]`` statistics of a masked
    ``table_moments(..., diffs=True)`` and the outputs of ``table_spectrum``."""
    if stats.dim() != 2 or stats.shape[0] != 12 or stats.dtype != torch.float64 or not stats.is_contiguous():
        raise ValueError("table_features: stats must be the contiguous fp64 [12, N] statistics of table_moments")
    N = stats.shape[1]
    out = _out_or_fresh("table_features", out, (N, 5), peak)
    check(_lib.load().ftn_table_features(_ptr(stats), _ptr(f_peak), _ptr(peak), _ptr(total), int(T), N, _ptr(out),
                                         _stream(stats.device)), "ftn_table_features")
    return out


def table_scaler(stats: torch.Tensor, method: str, per_series: bool = True, eps: float = 1e-8):
    """``ftn_table_scaler``: ``(loc [N], scale [N], pairs [2, N])`` fp32 from the unmasked statistics of
    ``table_moments``; the reference's ``eps`` rule, on the device."""
    if method not in TABLE_METHODS:
        raise ValueError(f"table_scaler: method {method!r} is not 'zscore' or 'minmax'")
    if stats.dim() != 2 or stats.shape[0] not in (6, 12) or stats.dtype != torch.float64 or not stats.is_contiguous():
        raise ValueError("table_scaler: stats must be the contiguous fp64 [6, N] statistics of table_moments")
    N, dev = stats.shape[1], stats.device
    loc = torch.empty(N, dtype=torch.float32, device=dev)
    scale = torch.empty(N, dtype=torch.float32, device=dev)
    pairs = torch.empty(2, N, dtype=torch.float32, device=dev)
    check(_lib.load().ftn_table_scaler(_ptr(stats), N, TABLE_METHODS[method], int(bool(per_series)), float(eps),
                                       _ptr(loc), _ptr(scale), _ptr(pairs), _stream(dev)), "ftn_table_scaler")
    return loc, scale, pairs


def _collapse(shape, strides):
    """``(size, stride)`` of consecutive dims read as one, or None when no single stride walks them."""
    dims = [(n, s) for n, s in zip(shape, strides) if n != 1]
    size = 1
    for n, _ in dims:
        size *= n
    if not dims:
        return 1, 0
    for (_, s0), (n1, s1) in zip(dims[:-1], dims[1:]):
        if s0 != s1 * n1:
            return None
    return size, dims[-1][1]


def _affine_view(t: torch.Tensor, axis: int):
    """``(outer, S, inner, outer stride, series stride)`` of ``t`` read as [outer][S][inner] around ``axis``, or None."""
    shape, strides = tuple(t.shape), tuple(t.stride())
    outer, inner = _collapse(shape[:axis], strides[:axis]), _collapse(shape[axis + 1:], strides[axis + 1:])
    if outer is None or inner is None or (inner[0] > 1 and inner[1] != 1):
        return None
    S, ss = shape[axis], strides[axis]
    if S > 1 and ss < inner[0]:
        return None
    if outer[0] > 1 and outer[1] < 0:
        return None
    return outer[0], S, inner[0], (outer[1] if outer[0] > 1 else 0), (ss if S > 1 else inner[0])


def table_affine_form_of(outer: int, S: int, inner: int, x_strides=None, o_strides=None, n_cols: int | None = None,
                         series: bool = False, inverse: bool = False, misalign: dict | None = None) -> dict:
    """The form ``ftn_table_affine`` takes (``ftn_table_affine_form``, host-only) over [outer][S][inner]:
    ``load_bytes`` 16 or 4, ``lane_axis`` 1 (four elements of one series), 2 (of four series) or 0, ``block`` elements
    a unit.  ``x_strides`` / ``o_strides``: (outer, series) element strides (default: dense)."""
    mis = dict(misalign or {})
    a = _lib.FtnTableAffineArgs()
    a.outer, a.S, a.inner = int(outer), int(S), int(inner)
    a.x_ostride, a.x_sstride = x_strides if x_strides is not None else (a.S * a.inner, a.inner)
    a.o_ostride, a.o_sstride = o_strides if o_strides is not None else (a.S * a.inner, a.inner)
    a.n_cols = int(S if n_cols is None else n_cols)
    a.flags = _lib.FTN_TAB_INVERSE if inverse else 0
    a.x, a.out = 0x100000 + mis.pop("x", 0), 0x200000 + mis.pop("out", 0)
    a.loc, a.scale, a.series = 0x300000, 0x400000, (0x500000 if series else None)
    if mis:
        raise ValueError(f"table_affine_form_of: misalign names {sorted(mis)} are not operands of the call")
    return _table_form("ftn_table_affine_form", a)


def table_affine(x: torch.Tensor, loc: torch.Tensor, scale: torch.Tensor, axis: int = -1, series=None,
                 inverse: bool = False, clip: bool = False, out: torch.Tensor | None = None, form: bool = False):
    """``ftn_table_affine``: ``(x - loc[c]) / scale[c]`` (``clip``: of ``max(x, 0)``) or, with ``inverse``,
    ``x * scale[c] + loc[c]`` (``clip``: then ``max(., 0)``) with the series along ``axis`` of the fp32 device tensor
    ``x``; ``c`` is the position along ``axis`` or ``series[position]`` (int64 on the device).  ``out`` may be ``x``
    or a tensor of x's shape; a view that one outer and one series stride cannot walk is an error for ``out`` and a
    contiguous copy for ``x``.  One launch on the current stream."""
    who = "table_affine"
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or not x.is_cuda or x.dim() < 1:
        raise ValueError(f"{who}: x must be an fp32 tensor on a ROCm device")
    axis = axis % x.dim()
    dev, n_cols = x.device, loc.numel()
    for name, t in (("loc", loc), ("scale", scale)):
        if t.dim() != 1 or t.dtype != torch.float32 or t.device != dev or not t.is_contiguous() or t.numel() != n_cols:
            raise ValueError(f"{who}: {name} must be a contiguous fp32 vector beside x")
    S = x.shape[axis]
    if series is not None:
        if (not isinstance(series, torch.Tensor) or series.shape != (S,) or series.dtype != torch.int64
                or series.device != dev or not series.is_contiguous()):
            raise ValueError(f"{who}: series must be a contiguous int64 [{S}] tensor beside x")
    elif S > n_cols:
        raise ValueError(f"{who}: {S} series along axis {axis} but loc and scale hold {n_cols}")
    if out is None:
        out = torch.empty(x.shape, dtype=torch.float32, device=dev)
    elif not isinstance(out, torch.Tensor) or out.shape != x.shape or out.dtype != torch.float32 or out.device != dev:
        raise ValueError(f"{who}: out must be an fp32 tensor of x's shape {tuple(x.shape)} beside x")
    if x.numel() == 0:
        return out
    vo = _affine_view(out, axis)
    if vo is None:
        raise ValueError(f"{who}: out with strides {out.stride()} cannot be walked as [outer][series][inner]")
    vx = _affine_view(x, axis)
    if vx is None:
        x = x.contiguous()
        vx = _affine_view(x, axis)
    a = _lib.FtnTableAffineArgs()
    a.x, a.out = _ptr(x), _ptr(out)
    a.outer, a.S, a.inner, a.x_ostride, a.x_sstride = vx
    a.o_ostride, a.o_sstride = vo[3], vo[4]
    if vo[0] > 1 and a.o_ostride == 0:
        raise ValueError(f"{who}: out repeats its rows (stride 0)")
    a.n_cols, a.flags = n_cols, (_lib.FTN_TAB_INVERSE if inverse else 0) | (_lib.FTN_TAB_CLIP if clip else 0)
    a.loc, a.scale, a.series = _ptr(loc), _ptr(scale), _ptr_or_null(series)
    if form:
        return _table_form("ftn_table_affine_form", a)
    check(_lib.load().ftn_table_affine(C.byref(a), _stream(dev)), "ftn_table_affine")
    return out


# ------------------------------------------------------------------ LRTC
def lrtc_form_of(N: int, R: int, addx: bool = False, misalign_or: int = 0) -> Tuple[str, bool, int]:
    """The kernel ``ftn_lrtc_forward`` runs for N series at rank R (``ftn_lrtc_form``, host-only: the launch
    dispatches through the same function): ``("k_lrtc<RT,VEC,ADDX>", wide coefficient loads, nqb)``.
    ``misalign_or``: ``((out | x) & 15) | (coeff & 15) << 4`` of the byte addresses."""
    f = _form("ftn_lrtc_form", N, R, addx, misalign_or)
    tf = ("false", "true")
    return f"k_lrtc<{(f >> 4) & 63},{tf[f & 1]},{tf[(f >> 1) & 1]}>", bool(f & 4), 64 * (f >> 12)


def lrtc_form(coeff: torch.Tensor, x: torch.Tensor | None = None, out: torch.Tensor | None = None):
    """``lrtc_form_of`` for the tensors ``lrtc_forward(coeff, L, scale, x)`` is given (its own ``out`` is a fresh,
    aligned tensor; ``out``: the one a direct ``ftn_lrtc_forward`` call would pass)."""
    mis = ((_ptr(out) if out is not None else 0) | (_ptr(x) if x is not None else 0)) & 15 | (_ptr(coeff) & 15) << 4
    return lrtc_form_of(coeff.shape[1], coeff.shape[2], x is not None, mis)


def lrtc_forward(coeff: torch.Tensor, L: int, scale: torch.Tensor, x: torch.Tensor | None) -> torch.Tensor:
    """``(x +) scale * (basis - colmean) coeff^T``: ``coeff`` [B,N,R] and the optional ``x`` [B,L,N] contiguous fp32
    on one device, ``scale`` one fp32 element there.  Returns [B,L,N]."""
    lib = _lib.load()
    if coeff.dim() != 3 or coeff.dtype != torch.float32 or not coeff.is_cuda or not coeff.is_contiguous():
        raise ValueError("lrtc_forward takes coeff as a contiguous fp32 device tensor [B, N, R]")
    B, N, R = coeff.shape
    if x is not None and (x.shape != (B, int(L), N) or x.dtype != torch.float32 or x.device != coeff.device
                          or not x.is_contiguous()):
        raise ValueError(f"lrtc_forward: x must be contiguous fp32 [B, L, N] = {(B, int(L), N)} beside coeff, "
                         f"got {tuple(x.shape)} {x.dtype} on {x.device}")
    if scale.numel() != 1 or scale.dtype != torch.float32 or scale.device != coeff.device:
        raise ValueError("lrtc_forward: scale must be one fp32 element beside coeff")
    st = state(coeff.device)
    basis = st.lrtc_basis(L, R)
    out = torch.empty(B, L, N, dtype=torch.float32, device=coeff.device)
    check(lib.ftn_lrtc_forward(_ptr(coeff), _ptr(basis), _ptr(scale), _ptr(x) if x is not None else None,
                               _ptr(out), B, L, N, R, _stream(coeff.device)), "ftn_lrtc_forward")
    return out


def selftest_mfma(device: torch.device) -> torch.Tensor:
    lib = _lib.load()
    out = torch.zeros(16, 16, dtype=torch.float32, device=device)
    check(lib.ftn_selftest_mfma(_ptr(out), _stream(device)), "ftn_selftest_mfma")
    return out
