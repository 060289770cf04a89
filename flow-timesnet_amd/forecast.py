"""Recursive forecasting with the state on the device.

``forecast_recursive_batch`` is a drop-in for the reference's ``predict.forecast_recursive_batch`` (predict.py:307-342):
H one-step forecasts, each fed back as the newest row of the next step's window.  The reference calls the whole model
H times from a host loop and rebuilds the ``[B, T, N]`` window with ``torch.cat`` between calls.  Here, for this
package's ``TimesNet`` in ``recursive`` mode on ROCm fp32 tensors without autograd, the loop keeps three pieces of
state on the device instead:

* ``V`` - a ring ``[B, L, D]`` of value-embedded rows ``x W^T`` (no bias, add or norm; L = ``input_len``).  Row t of
  ``x W^T`` depends only on row t of x, and everything else the embedding adds is indexed by position, so a step embeds
  only its B new rows (``ftn_embed_rows_strided``) and rebuilds the window's embedding in one memory-bound pass
  (``ftn_embed_ring``) with the one-pass embedding's epilogue arithmetic.
* the history tail - in recursive mode the heads read only the last observed row: ``last_seq[:, -1]`` on step 0, the
  previous step's rate afterwards;
* the mark window, if any - ``[B, L, time_dim]`` is small: sliced and concatenated per step.

Every step is enqueued without a host synchronisation; the finite-positive flags of the heads and the f16x2 range
flags of the blocks are collected for every step and read once after the forecast.  ``RecursiveForecaster`` captures
the whole unrolled H-step forecast as one HIP graph (every ring slot is a Python integer at capture time, so no device
counter is needed).  Both are bit-identical to the reference loop driven over the same model on the same device.

Anything else - CPU tensors, a ``direct``-mode model, autograd, d_model > 512 (> 128 under ``FTN_SHELL_WIDE=0``), a
foreign model, a ``last_seq`` whose window takes another embedding kernel than the loop's later
windows (a view that is not 16-byte aligned, or whose batch stride is not a multiple of 4, with N % 4 == 0),
``embed_norm_mode="layer"`` at a d_model <= 128 that is not a multiple of 16 or on a form outside
``RING_EXACT_LAYER_FORMS`` - runs the reference's loop unchanged (``forecast_recursive_batch_loop``).  Beyond d_model 128
the wide embedding and the wide ring share one epilogue function compiled without FMA contraction, so all four wide
forms are in that set at every d_model.  ``embed_norm_mode="rms"`` carries no such condition: its epilogue is compiled
without FMA contraction in the narrow kernels too, so the ring is bit-identical to the one-pass embedding on every form
and at every d_model.

``forecast_sample_paths`` is the same recursion fed with draws instead of rates (``score.nb_sample`` at
``offset = step``), P paths as one batch of P B rows; ``forecast_sample_paths_loop`` fixes its semantics.
"""
from __future__ import annotations

import contextlib
from typing import Any, Dict, List, Optional, Tuple

import torch

from . import range_guard

_MISSING_Y_MARK = "Temporal features provided for history but missing future marks during recursive forecast"
_SHORT_Y_MARK = "y_mark does not provide enough future steps for recursive forecasting"
_RANGE_WARNING = ("TimesBlock: a value left the fp16 range of engine f16x2 (|v| >= 65504 or not finite) during a "
                  "recursive forecast; the forecast was repeated with every block on engine bf16x3")


# embedding forms whose LayerNorm epilogue is bit-identical to k_embed_ring's at d_model % 16 == 0: the default forms
# bar the fp32-MFMA one of d_model > 64 (k_embed_in<8, *>); the forms behind FTN_EMBED_F32 / FTN_EMBED_RT are not
# (k_embed_in_bf<8,2> differs in the last bit) or not established
_WIDE_FORMS = frozenset(f"k_embed_wide_bf<{no},4,{vec}>" for no in (4, 8) for vec in ("true", "false"))   # exact at every d_model
RING_EXACT_LAYER_FORMS = frozenset({"k_embed_in_bf<4,2>", "k_embed_in_bf<8,1>", "k_embed_in<4,false>"}) | _WIDE_FORMS


def _invoke_model(model, xb, x_mark=None, series_static=None, series_ids=None):
    """The reference's ``_invoke_model`` (predict.py:261-295): only the given keyword arguments are passed, and a
    model that rejects one of them is called again without it."""
    kwargs: Dict[str, torch.Tensor] = {}
    if x_mark is not None:
        kwargs["x_mark"] = x_mark
    if series_static is not None:
        kwargs["series_static"] = series_static
    if series_ids is not None:
        kwargs["series_ids"] = series_ids
    try:
        return model(xb, **kwargs)
    except TypeError as err:
        err_str = str(err)
        for key in ["series_static", "series_ids", "x_mark"]:
            if key in kwargs and key in err_str:
                kwargs.pop(key)
                try:
                    return model(xb, **kwargs)
                except TypeError as inner_err:
                    err_str = str(inner_err)
                    continue
        raise


def forecast_recursive_batch_loop(model, last_seq, H, x_mark=None, y_mark=None, series_static=None,
                                  series_ids=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The reference's host loop (predict.py:307-342), unchanged."""
    rates: List[torch.Tensor] = []
    dispersions: List[torch.Tensor] = []
    seq = last_seq
    mark_seq = x_mark
    for step in range(H):
        rate_step, dispersion_step = _invoke_model(model, seq, x_mark=mark_seq, series_static=series_static,
                                                   series_ids=series_ids)
        rates.append(rate_step)
        dispersions.append(dispersion_step)
        seq = torch.cat([seq[:, 1:, :], rate_step], dim=1)
        if mark_seq is not None:
            if y_mark is None:
                raise ValueError(_MISSING_Y_MARK)
            if y_mark.size(1) <= step:
                raise ValueError(_SHORT_Y_MARK)
            next_mark = y_mark[:, step: step + 1, :]
            mark_seq = torch.cat([mark_seq[:, 1:, :], next_mark], dim=1)
    return torch.cat(rates, dim=1), torch.cat(dispersions, dim=1)


# ---------------------------------------------------------------------------------------------------------- device path
def _shapes_ok(model, last_seq, H, x_mark, y_mark) -> bool:
    """The inputs are well formed for the device path (anything else goes to the loop, which raises the reference's
    errors where it has them)."""
    from .models.shell import TimesNet

    if type(model) is not TimesNet or model.mode != "recursive" or model.training:
        return False
    if not isinstance(last_seq, torch.Tensor) or last_seq.dim() != 3 or int(H) < 1:
        return False
    B, T, N = last_seq.shape
    L = model.input_len
    if T < L or L < 1 or B < 1 or N < 1 or torch.is_grad_enabled():
        return False
    tensors = [last_seq] + [m for m in (x_mark, y_mark) if m is not None]
    if any(not t.is_cuda or t.dtype != torch.float32 or t.device != last_seq.device for t in tensors):
        return False
    if x_mark is not None:
        if x_mark.dim() != 3 or tuple(x_mark.shape[:2]) != (B, T):
            return False
        if y_mark is not None and (y_mark.dim() != 3 or y_mark.size(0) != B or y_mark.size(2) != x_mark.size(2)):
            return False
    return True


def _check_marks(x_mark, y_mark, H) -> None:
    """The reference's two ValueErrors (raised by its loop after the first model call; here before any)."""
    if x_mark is not None:
        if y_mark is None:
            raise ValueError(_MISSING_Y_MARK)
        if y_mark.size(1) < H:
            raise ValueError(_SHORT_Y_MARK)


def _prepare(model, last_seq, x_mark, series_static, series_ids):
    """Lazy layers built / placed as the first step of the loop would; returns whether the HIP embedding and heads
    take this model and these tensors."""
    L = model.input_len
    window = last_seq.narrow(1, last_seq.size(1) - L, L)
    mark = None if x_mark is None else x_mark.narrow(1, x_mark.size(1) - L, L)
    model._ensure_embedding(window, mark, series_static, series_ids)
    tail = last_seq[:, -1:, :]
    if not (model._hip_embed_ok(window) and model._hip_heads_ok(tail, tail)):
        return False
    # The ring holds the step-0 rows as the first window's kernel form computed them, while the loop re-embeds them at
    # every step from a fresh torch.cat - an aligned view with batch stride T * N.  The forms differ when the first
    # window is not 16-byte aligned or has a batch stride that is not a multiple of 4 while N % 4 == 0 (fp32 MFMA
    # first, bf16x3 afterwards): not bit-identical, so the loop runs.  The library's own rule decides (embed_form).
    from . import runtime

    w = model.embedding.value_embedding.weight.detach()
    B, T, N = last_seq.shape
    form = runtime.embed_form(window, w)
    if form != runtime.embed_form_at(N, w.size(0), T * N if B > 1 else 0, 0, w.data_ptr() & 15):
        return False
    # "layer" mode: the compiler contracts the LayerNorm epilogue of the GEMM kernels into FMAs differently from
    # k_embed_ring's on some forms, and on every form at a d_model that is not a multiple of 16 (partly masked column
    # tiles).  The ring is then equal to the loop up to rounding only, so it is used for the forms
    # whose bit-identity the GPU suite establishes and the loop runs for the rest.  The "rms" epilogue is compiled
    # without contraction in every kernel: no form condition
    if model.embedding.embed_norm_mode != "layer":
        return True
    return form in RING_EXACT_LAYER_FORMS and (model.d_model % 16 == 0 or form in _WIDE_FORMS)


def _device_ok(model, last_seq, H, x_mark, y_mark, series_static, series_ids) -> bool:
    if not _shapes_ok(model, last_seq, H, x_mark, y_mark):
        return False
    _check_marks(x_mark, y_mark, H)
    return _prepare(model, last_seq, x_mark, series_static, series_ids)


def _mark_window(x_mark, y_mark, L: int, s: int) -> torch.Tensor:
    """The loop's mark window after s >= 1 steps: the last L rows of ``cat(x_mark[:, s:], y_mark[:, :s])``, built as
    the loop builds it (a [B, T, time_dim] sequence, then a view) so the time-feature GEMM sees the same layout."""
    T = x_mark.size(1)
    seq = torch.cat([x_mark[:, min(s, T):], y_mark[:, max(0, s - T):s]], dim=1)
    return seq.narrow(1, T - L, L)


def _enqueue(model, last_seq, H, x_mark, y_mark, series_static, series_ids, rate_out, disp_out, feedback=None):
    """Enqueue the H steps (no host synchronisation).  Writes step s into ``[:, s]`` of the outputs; returns the heads'
    finite-positive flags (one per step).  ``feedback(s, rate, disp)`` gives the row [B, 1, N] that step s feeds back as
    the newest observation; the default is the rate itself, the reference's recursion."""
    from . import runtime

    L = model.input_len
    T = last_seq.size(1)
    window = last_seq.narrow(1, T - L, L)
    mark0 = None if x_mark is None else x_mark.narrow(1, T - L, L)
    model._ensure_embedding(window, mark0, series_static, series_ids)
    rows = model._context_rows(window, series_static, series_ids)
    coeff, bias = model._context_terms(rows)
    w, add, ln = model._hip_embed_terms(window, mark0, coeff, bias)
    B, N, D = window.size(0), window.size(2), w.size(0)
    V = torch.empty(B, L, D, dtype=torch.float32, device=window.device)
    runtime.embed_rows_strided(window, w, V, 0)
    tail = last_seq[:, -1:, :]
    bads = []
    for s in range(H):
        if s > 0:
            runtime.embed_rows_strided(tail, w, V, (s - 1) % L)
            if x_mark is not None:
                _, add, _ = model._hip_embed_terms(window, _mark_window(x_mark, y_mark, L, s), coeff, bias)
        seq = model._stack(runtime.embed_ring(V, s % L, add, ln))
        rate, disp = model._heads(seq, tail, rows, 1)
        bads.append(model._pending_bad)
        rate_out[:, s].copy_(rate[:, 0])
        disp_out[:, s].copy_(disp[:, 0])
        tail = rate if feedback is None else feedback(s, rate, disp)
    model._last_embed_backend = "hip"
    return bads


@contextlib.contextmanager
def _deferred_checks(model):
    """The model's finite-positive check is left to the caller for the length of one forecast (and its ids check,
    which reads the device, is skipped, as in a capture)."""
    saved = model._defer_checks
    model._defer_checks = True
    try:
        yield
    finally:
        model._defer_checks = saved
        model._pending_bad = None


def _raise_if_bad(bads) -> None:
    """The reference's RuntimeError (timesnet.py:2095-2098) for the first step whose rate or dispersion is not finite
    and > 0, as its loop would have raised it at that step."""
    bads = [b for b in bads if b is not None]
    if not bads:
        return
    for flag in torch.stack([b.reshape(()) for b in bads]).tolist():
        for bit, name in ((1, "rate"), (2, "dispersion")):
            if flag & bit:
                raise RuntimeError(f"Predicted {name} must be finite and strictly positive")


def _forecast_device(model, last_seq, H, x_mark, y_mark, series_static, series_ids):
    """The blocks' f16x2 range flags of all H steps are read once, after the forecast (``range_guard``)."""
    def run():
        rate = torch.empty(last_seq.size(0), H, last_seq.size(2), dtype=torch.float32, device=last_seq.device)
        disp = torch.empty_like(rate)
        bads = _enqueue(model, last_seq, H, x_mark, y_mark, series_static, series_ids, rate, disp)
        return rate, disp, bads

    with _deferred_checks(model):
        rate, disp, bads = range_guard.repeat_on_trip(model.blocks, run, message=_RANGE_WARNING)
    _raise_if_bad(bads)
    return rate, disp


def forecast_recursive_batch(model, last_seq: torch.Tensor, H: int, x_mark: Optional[torch.Tensor] = None,
                             y_mark: Optional[torch.Tensor] = None, series_static: Optional[torch.Tensor] = None,
                             series_ids: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Drop-in for the reference's ``forecast_recursive_batch``: ``(rate[B, H, N], dispersion[B, H, N])``.  Runs on
    the device (see the module docstring) when it can, the reference's loop otherwise."""
    if _device_ok(model, last_seq, H, x_mark, y_mark, series_static, series_ids):
        return _forecast_device(model, last_seq, int(H), x_mark, y_mark, series_static, series_ids)
    return forecast_recursive_batch_loop(model, last_seq, H, x_mark, y_mark, series_static, series_ids)


# --------------------------------------------------------------------------------------------------------- sample paths
def _repeat_paths(P, B, last_seq, x_mark, y_mark, series_static, series_ids):
    """The inputs of a batch of P B rows, path-major (row p B + b): what has a batch axis is repeated P times."""
    def rep(t, batched):
        return t if t is None or not batched else t.repeat(P, *([1] * (t.dim() - 1)))

    return (rep(last_seq, True), rep(x_mark, True), rep(y_mark, True),
            rep(series_static, series_static is not None and series_static.dim() == 3 and series_static.size(0) == B),
            rep(series_ids, series_ids is not None and series_ids.dim() == 2 and series_ids.size(0) == B))


def _raise_if_sample_range(flags) -> None:
    for step, flag in enumerate(flags.tolist()):
        if flag:
            raise RuntimeError(f"forecast_sample_paths: a draw of step {step} is outside the supported range "
                               f"[0, 2^24) (its rate or dispersion is too large to sample)")


def forecast_sample_paths_loop(model, last_seq, H, n_paths, seed=0, x_mark=None, y_mark=None, series_static=None,
                               series_ids=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """What ``forecast_sample_paths`` means, as a host loop: the P paths of the B rows are the rows of one batch of
    P B (path-major); step s calls the model on that batch, draws ``score.nb_sample(rate_s, disp_s, 1, seed,
    offset=s)[0]`` and feeds the draw - not the rate - back as the newest row of every path's window."""
    from . import score

    P, B = int(n_paths), last_seq.size(0)
    if P < 1 or int(H) < 1:
        raise ValueError(f"forecast_sample_paths: n_paths={n_paths}, H={H}")
    seq, mark_seq, y_mark, series_static, series_ids = _repeat_paths(P, B, last_seq, x_mark, y_mark, series_static,
                                                                     series_ids)
    samples: List[torch.Tensor] = []
    rates: List[torch.Tensor] = []
    dispersions: List[torch.Tensor] = []
    for step in range(int(H)):
        rate_step, dispersion_step = _invoke_model(model, seq, x_mark=mark_seq, series_static=series_static,
                                                   series_ids=series_ids)
        flag = torch.zeros(1, dtype=torch.int32, device=rate_step.device)
        with torch.no_grad():
            draw = score.nb_sample(rate_step.detach().float(), dispersion_step.detach().float(), 1, seed, offset=step,
                                   flag=flag)[0]
        _raise_if_sample_range(flag)
        samples.append(draw)
        rates.append(rate_step)
        dispersions.append(dispersion_step)
        seq = torch.cat([seq[:, 1:, :], draw.to(seq.dtype)], dim=1)
        if mark_seq is not None:
            if y_mark is None:
                raise ValueError(_MISSING_Y_MARK)
            if y_mark.size(1) <= step:
                raise ValueError(_SHORT_Y_MARK)
            mark_seq = torch.cat([mark_seq[:, 1:, :], y_mark[:, step: step + 1, :]], dim=1)
    N = last_seq.size(2)
    return tuple(torch.cat(v, dim=1).reshape(P, B, int(H), N) for v in (samples, rates, dispersions))


def _sample_paths_device(model, seq, H, seed, x_mark, y_mark, series_static, series_ids):
    """``_forecast_device`` with the draw fed back: the sample range flags of all H steps are one device vector, read
    after the forecast with the heads' and the blocks' flags."""
    from . import score

    def run():
        rate = torch.empty(seq.size(0), H, seq.size(2), dtype=torch.float32, device=seq.device)
        disp, samples = torch.empty_like(rate), torch.empty_like(rate)
        flags = torch.zeros(H, dtype=torch.int32, device=seq.device)

        def feedback(s, rate_s, disp_s):
            draw = score.nb_sample(rate_s, disp_s, 1, seed, offset=s, backend="hip", flag=flags[s:s + 1])[0]
            samples[:, s].copy_(draw[:, 0])
            return draw

        bads = _enqueue(model, seq, H, x_mark, y_mark, series_static, series_ids, rate, disp, feedback)
        return samples, rate, disp, bads, flags

    with _deferred_checks(model):
        samples, rate, disp, bads, flags = range_guard.repeat_on_trip(model.blocks, run, message=_RANGE_WARNING)
    _raise_if_sample_range(flags)           # a draw out of range is a NaN in the next window: the cause comes first
    _raise_if_bad(bads)
    return samples, rate, disp


def forecast_sample_paths(model, last_seq: torch.Tensor, H: int, n_paths: int, seed=0,
                          x_mark: Optional[torch.Tensor] = None, y_mark: Optional[torch.Tensor] = None,
                          series_static: Optional[torch.Tensor] = None, series_ids: Optional[torch.Tensor] = None
                          ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``n_paths`` sample paths of an H-step recursive forecast: ``(samples, rate, dispersion)``, each [P, B, H, N].
    Path p of row b draws its step-s count from the model's distribution given its own earlier draws, so the spread
    of ``samples[:, b, s]`` grows with s as the forecast's uncertainty does; ``rate`` and ``dispersion`` are the
    distributions each path drew from.  ``score.path_summary`` turns the paths into intervals, means and CRPS scores of
    window sums (``reduce="sum"``) and window maxima (``path_summary(..., reduce="max")``) on the device.

    The semantics are ``forecast_sample_paths_loop``'s, bit for bit.  The paths are the rows of one batch of P B, and
    the period selector averages amplitudes over its batch, so the paths see each other through the selected periods
    (and a forecast with other ``n_paths`` is not a prefix of this one): that is the model's own behaviour on such a
    batch.  A draw is a pure function of ``(seed, step, row, series)`` and the step's distribution
    (``score.nb_sample`` at ``offset = step``).  Runs on the device, without a host synchronisation per step, where
    ``forecast_recursive_batch`` would for the repeated batch; the loop otherwise.  A draw outside [0, 2^24) raises a
    RuntimeError that names its step."""
    P = int(n_paths)
    if P < 1 or int(H) < 1:
        raise ValueError(f"forecast_sample_paths: n_paths={n_paths}, H={H}")
    if isinstance(last_seq, torch.Tensor) and last_seq.dim() == 3:
        B, N = last_seq.size(0), last_seq.size(2)
        seq, xm, ym, st, ids = _repeat_paths(P, B, last_seq, x_mark, y_mark, series_static, series_ids)
        seed_ok = not isinstance(seed, torch.Tensor) or seed.device == last_seq.device
        if seed_ok and _device_ok(model, seq, H, xm, ym, st, ids):
            out = _sample_paths_device(model, seq, int(H), seed, xm, ym, st, ids)
            return tuple(t.view(P, B, int(H), N) for t in out)
    return forecast_sample_paths_loop(model, last_seq, H, n_paths, seed, x_mark, y_mark, series_static, series_ids)


# --------------------------------------------------------------------------------------------------------- graph replay
class RecursiveForecaster:
    """``fc = RecursiveForecaster(model, last_seq, H, x_mark=..., y_mark=..., series_static=..., series_ids=...)``
    captures the whole H-step device forecast as one HIP graph; ``fc(last_seq, x_mark=..., y_mark=...)`` copies the
    new inputs into the captured buffers, replays, checks, and returns the captured output tensors (overwritten by the
    next call).  As ``graph.GraphedForward``: shapes, H and the static features / ids are frozen at capture time.

    After a replay the blocks' range flags are read; if a value left the f16x2 range, every block is put on bf16x3,
    the forecast is captured again and replayed, so the caller never receives an unrepaired forecast.  Then the
    reference's finite-positive RuntimeError is raised if any step produced a bad rate or dispersion."""

    def __init__(self, model, last_seq: torch.Tensor, H: int, x_mark: Optional[torch.Tensor] = None,
                 y_mark: Optional[torch.Tensor] = None, series_static: Optional[torch.Tensor] = None,
                 series_ids: Optional[torch.Tensor] = None) -> None:
        self.model = model.eval()
        self.H = int(H)
        with torch.inference_mode():
            if not _device_ok(model, last_seq, self.H, x_mark, y_mark, series_static, series_ids):
                raise ValueError("RecursiveForecaster needs this package's TimesNet in recursive mode, ROCm fp32 "
                                 "inputs, and an embedding / heads the HIP kernels take")
            self._in = tuple(None if t is None else t.clone() for t in (last_seq, x_mark, y_mark))
            # on the device: a capture cannot copy from pageable host memory
            self._ctx = tuple(None if t is None else t.to(last_seq.device).clone() for t in (series_static, series_ids))
            self._capture()

    def _capture(self) -> None:
        model, (seq, xm, ym), (st, ids) = self.model, self._in, self._ctx
        dev = seq.device
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side), torch.inference_mode():          # lazy builds, weight packs, tables, workspace
            _forecast_device(model, seq, self.H, xm, ym, st, ids)
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        B, N = seq.size(0), seq.size(2)
        self.graph = torch.cuda.CUDAGraph()
        with torch.inference_mode():
            self._rate = torch.empty(B, self.H, N, dtype=torch.float32, device=dev)
            self._disp = torch.empty_like(self._rate)
            with _deferred_checks(model), range_guard.device_flags(model.blocks) as self._flags, \
                    torch.cuda.graph(self.graph):
                self._bads = _enqueue(model, seq, self.H, xm, ym, st, ids, self._rate, self._disp)
        self._sel = model.period_selector._pending          # the last step's period selection (device descriptor)
        # the captured launches have the packed weight blobs' addresses baked in: keep them alive
        self._packs = [m._pack for m in model.modules() if getattr(m, "_pack", None) is not None]

    @property
    def inputs(self) -> Tuple[Any, ...]:
        """The captured ``(last_seq, x_mark, y_mark)`` buffers (None where not given); writing into them directly saves
        the copy in ``__call__``."""
        return self._in

    def replay(self) -> Tuple[torch.Tensor, torch.Tensor]:
        while True:
            self.graph.replay()
            if not range_guard.tripped(self._flags):
                break
            range_guard.fall_back(self.model.blocks, _RANGE_WARNING)
            self._capture()                               # every block is on bf16x3 now
        _raise_if_bad(self._bads)
        if self._sel is not None:
            self._sel._host = None                        # the replay rewrote the descriptor
            self.model.period_selector._pending = self._sel
        return self._rate, self._disp

    def __call__(self, last_seq: torch.Tensor, x_mark: Optional[torch.Tensor] = None,
                 y_mark: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        for dst, src, name in zip(self._in, (last_seq, x_mark, y_mark), ("last_seq", "x_mark", "y_mark")):
            if (dst is None) != (src is None):
                raise ValueError(f"RecursiveForecaster: {name} must be given exactly when it was at capture time")
            if dst is None:
                continue
            if src.shape != dst.shape or src.dtype != dst.dtype:
                raise ValueError("RecursiveForecaster: input does not match the captured shape/dtype")
            if src.data_ptr() != dst.data_ptr():
                dst.copy_(src, non_blocking=True)
        return self.replay()
