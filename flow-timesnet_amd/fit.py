"""Adapting a checkpoint to new data under the model's own loss: the negative-binomial likelihood of the reference's
``losses.py`` with its gradient in closed form.

``nb_nll_grad`` returns the loss and its gradients with respect to rate and dispersion; ``negative_binomial_nll`` has
the reference's name and signature and is differentiable in both through them (a ``torch.autograd.Function``: autograd
records one node, not the formula).  Per element, with ``yc = max(y, 0)``, ``mu = max(rate, eps)``,
``alpha = max(dispersion, eps)``, the log-likelihood's derivatives are

    g_rate = (yc - mu) / (mu (1 + alpha mu))
    g_disp = (log1p(alpha mu) - [psi(yc + 1/alpha) - psi(1/alpha)]) / alpha^2 + (yc - mu) / (alpha (1 + alpha mu))

and the gradients of the loss are these times ``-1 / max(valid elements, 1)``, 0 where the clamp at ``eps`` is active
and where an element is masked out or not finite (``score.negative_binomial_mask``).  The second formula cancels to a
remainder ``1 / (alpha mu)`` below its terms, which is why fp32 autograd of the reference's formula has a median
relative error of 4e-2 in the dispersion gradient just above the default floor ``min_sigma = 1e-3`` (DESIGN.md
section 4, "Head refit").  Both backends evaluate it in fp64 and take the digamma difference from one well-conditioned
expansion (``sc_dpsi`` in ``csrc/ftn_nbmath.h``, ``_dpsi`` here):

* ``hip``: ``ftn_nb_nll_grad`` (``csrc/headfit.hip``) for fp32 [B,H,N] tensors on a ROCm device, fp32 in and out,
  no synchronisation; ``_last_backend`` records which ran;
* ``torch``: the same closed forms in fp64 torch ops, on any device; the loss itself is the reference's fp32
  function with the invalid elements left out.

``head_nll`` is the heads plus that loss on the ``hidden`` rows ``TimesNet.head_inputs`` returns, and ``refit_heads``
the loop ``head_inputs`` -> ``head_nll`` -> ``backward()`` -> a torch optimizer over ``mu_head`` and ``sigma_head``
alone: the backbone runs frozen on the HIP path (every block's ``_last_backend`` reads ``"hip"``) and a step is four
kernels - ``ftn_head_fit_forward`` (the heads, keeping softplus' derivative at both pre-activations),
``ftn_nb_nll_grad`` (raw derivatives, loss and scale word) and ``ftn_head_backward`` (row chunks, then their ordered
sum).  On tensors those kernels do not take (CPU, other dtypes) ``head_nll`` is the torch composition of the heads
with the loss node; ``_last_head_backend`` says which ran.

``time_projection`` is ``forecast_time_proj`` as a node of its own (``ftn_timeproj_forward`` forward,
``ftn_timeproj_backward`` in ``csrc/timeproj_bwd.hip`` backward, on the ``seq`` rows ``TimesNet.output_inputs``
returns), ``output_nll`` that node followed by ``head_nll``, and ``refit_output`` the loop of ``refit_heads`` over the
whole output side: the time projection and both heads, with the reference's gradient clipping when asked.  The
backbone stays frozen on the HIP path and every gradient comes from this library's kernels, in a fixed summation
order; ``_last_timeproj_backend`` says which path the projection took.

``DeviceAdamW`` is the optimizer of that loop with nothing on the host: torch's ``clip_grad_norm_`` followed by torch's
AdamW as one call of ``ftn_refit_update`` (``csrc/refit.hip``), whose step count, learning rate, gradient norm and
decision to skip a step are device words.  ``GraphedRefitStep`` captures a whole step of ``refit_output`` - backbone
forward, time projection, heads, loss, both backwards, that update - in one HIP graph, and ``refit_output_graphed`` is
the loop over it ("Refit step").

``OutputCache`` keeps what the output side reads of a frozen backbone - ``seq`` first of all - per item of a
``windows.DeviceWindows``; ``GraphedCachedStep`` is ``GraphedRefitStep`` without the blocks, reading the cached ``seq``
in place through a device row list (``time_projection(..., rows=)``, the ``_rows`` entries of ``csrc/timeproj.hip`` and
``csrc/timeproj_bwd.hip``; ``ftn_refit_rows_gather`` for the rest of the batch), and ``refit_output_cached`` the loop
over shuffled epochs ("Cached refit").

``refit_output_validated`` is that loop with the reference's per-epoch validation decided on the device:
``GraphedCachedEval`` scores held-out windows from an ``OutputCache`` of their own into ``ValidationAccumulators``,
and ``EpochEnd`` (``ftn_refit_epoch_end``, ``csrc/refit_epoch.hip``) turns the sums into the validation NLL, steps
``ReduceLROnPlateau`` in the optimizer's ``lr`` word, keeps the best epoch's tensors and sets the stop word that every
later step takes as a skip word ("Validated refit").

``late_bias`` is the late-bias head - the one per-series term behind the backbone - as an autograd node over
``ftn_late_fit_forward`` / ``ftn_late_backward`` (``csrc/latefit.hip``) on the frozen series rows
``TimesNet.late_rows`` returns; its result is the ``late=`` of ``head_nll`` / ``output_nll``.
``refit_output(..., late_bias=True)`` moves its five parameters with the six of the output side, and
``DeviceAdamWList`` is ``DeviceAdamW`` for up to 32 tensors over ``ftn_refit_update_list`` (DESIGN.md section 4,
"Late-bias refit").

``backend`` follows ``score``'s rule (``_use_hip``): ``hip`` where it can run unless ``"torch"`` is asked for, and
asking for ``"hip"`` where it cannot is an error.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from .score import (ForecastScorer, _full_mask, _nb_ll_torch, _part_views, _rows, _use_hip,
                    negative_binomial_mask)

_last_backend: Optional[str] = None
_last_head_backend: Optional[str] = None      # which path the last ``head_nll`` took


def _dpsi(y: torch.Tensor, r: torch.Tensor) -> torch.Tensor:
    """``psi(y + r) - psi(r)`` for fp64 ``y >= 0``, ``r > 0``: ``sc_dpsi`` step by step (both arguments go up by the
    same steps until ``r >= 8``, then the difference of the two asymptotic series term by term), so it is as accurate
    for ``r`` large against ``y`` as anywhere else, where two digammas subtracted lose ``log(r) r / y`` ulps."""
    R, s = r.clone(), torch.zeros_like(r)
    for _ in range(8):
        up = R < 8.0
        s = torch.where(up, s + y / (R * (R + y)), s)
        R = torch.where(up, R + 1.0, R)
    X = R + y
    a, b = 1.0 / R, 1.0 / X
    za, zb = a * a, b * b
    pb, h, g = zb, za + zb, torch.full_like(r, -1.0 / 12.0)
    for c in (1.0 / 120.0, -1.0 / 252.0, 1.0 / 240.0, -1.0 / 132.0):
        g = g + c * h
        pb = pb * zb
        h = za * h + pb
    return s + (torch.log1p(y * a) + y * a * b * (0.5 - (R + X) * a * b * g))


def _nb_grad_torch(y, rate, dispersion, mask, eps):
    """``(loss, g_rate, g_disp)``: the loss in the reference's own fp32 operations (losses.py:36-58 line by line, an
    invalid element left out instead of multiplied by 0), the gradients from the closed forms in fp64 torch ops on
    the same clamped fp32 values.  fp32 results."""
    ll32 = _nb_ll_torch(y, rate, dispersion, eps)[0]
    eps = torch.tensor(eps, dtype=torch.float32, device=y.device)   # the fp32 word the kernel compares with
    y32 = torch.clamp(y.to(torch.float32), min=0.0)
    al32 = torch.maximum(dispersion.to(torch.float32), eps)     # a NaN stays a NaN
    mu32 = torch.maximum(rate.to(torch.float32), eps)
    valid = negative_binomial_mask(y32, mu32, al32, mask)
    one = torch.ones((), dtype=torch.float64, device=y32.device)
    Y = torch.where(valid, y32.double(), 0.0 * one)             # an invalid element computes on harmless values
    A = torch.where(valid, al32.double(), one)
    M = torch.where(valid, mu32.double(), one)
    r, t = 1.0 / A, A * M
    l1p = torch.log1p(t)
    dq = (Y - M) / (1.0 + t)
    live_r = valid & ~(rate.to(torch.float32) < eps)
    live_d = valid & ~(dispersion.to(torch.float32) < eps)
    raw_r = torch.where(live_r, dq / M, 0.0 * one)
    raw_d = torch.where(live_d, (l1p - _dpsi(Y, r)) * r * r + dq * r, 0.0 * one)
    denom = torch.clamp(valid.sum(), min=1)
    loss = -torch.where(valid, ll32, torch.zeros((), device=ll32.device)).sum() / denom.to(torch.float32)
    scale = -1.0 / denom.to(torch.float64)
    return loss, (raw_r * scale).float(), (raw_d * scale).float()


def _hip_operands(*tensors) -> bool:
    """fp32 [B,H,N] tensors of one shape on one ROCm device, not empty (whether they require grad does not matter:
    nothing here is recorded)."""
    if not all(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 3
               for t in tensors):
        return False
    return (len({t.device for t in tensors}) == 1 and len({tuple(t.shape) for t in tensors}) == 1
            and tensors[0].numel() > 0)


def nb_nll_grad(y: torch.Tensor, rate: torch.Tensor, dispersion: torch.Tensor, mask: torch.Tensor | None = None,
                eps: float = 1e-8, backend: Optional[str] = None):
    """``(loss, g_rate, g_disp)``: the loss of ``negative_binomial_nll`` (a 0-dim fp32 tensor) and its gradients with
    respect to ``rate`` and ``dispersion`` (fp32, their shape).  Nothing is recorded for autograd."""
    global _last_backend
    for name, t in (("y", y), ("rate", rate), ("dispersion", dispersion)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"nb_nll_grad: {name} must be a tensor")
        if tuple(t.shape) != tuple(y.shape):
            raise ValueError(f"nb_nll_grad: {name} has shape {tuple(t.shape)}, y has {tuple(y.shape)}")
    if not 0.0 < float(eps) < 1.0:
        raise ValueError(f"nb_nll_grad: eps={eps} is not inside (0, 1)")
    if mask is not None:
        if not isinstance(mask, torch.Tensor):
            raise TypeError("nb_nll_grad: mask must be a tensor or None")
        if mask.ndim > y.ndim or not _broadcasts(mask, y):
            raise ValueError(f"nb_nll_grad: a mask of shape {tuple(mask.shape)} does not broadcast over "
                             f"{tuple(y.shape)}")
    y, rate, dispersion = y.detach(), rate.detach(), dispersion.detach()
    if _use_hip("nb_nll_grad", backend, _hip_operands(y, rate, dispersion),
                "fp32 [B, H, N] tensors of one shape on one ROCm device"):
        from . import runtime as rt

        words, g_rate, g_disp = rt.nb_nll_grad(_rows(y), _rows(rate), _rows(dispersion), _full_mask(mask, y), eps)
        _last_backend = "hip"
        return words[0], g_rate, g_disp
    _last_backend = "torch"
    return _nb_grad_torch(y, rate, dispersion, mask, float(eps))


def _broadcasts(mask: torch.Tensor, like: torch.Tensor) -> bool:
    """Whether ``negative_binomial_mask`` can expand ``mask`` over ``like``: trailing 1s are appended, then
    ``expand_as``."""
    shape = tuple(mask.shape) + (1,) * (like.ndim - mask.ndim)
    return all(m in (1, n) for m, n in zip(shape, like.shape))


class _NegativeBinomialNLL(torch.autograd.Function):
    """The loss as one autograd node whose backward is ``nb_nll_grad``'s gradients times the incoming one."""

    @staticmethod
    def forward(ctx, y, rate, dispersion, mask, eps, backend):
        loss, g_rate, g_disp = nb_nll_grad(y, rate, dispersion, mask, eps, backend)
        ctx.save_for_backward(g_rate, g_disp)
        ctx.dtypes = (rate.dtype, dispersion.dtype)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        g_rate, g_disp = ctx.saved_tensors
        return (None, (grad_out * g_rate).to(ctx.dtypes[0]), (grad_out * g_disp).to(ctx.dtypes[1]), None, None, None)


def negative_binomial_nll(y: torch.Tensor, rate: torch.Tensor, dispersion: torch.Tensor,
                          mask: torch.Tensor | None = None, eps: float = 1e-8,
                          backend: Optional[str] = None) -> torch.Tensor:
    """Negative binomial negative log-likelihood averaged over the valid elements (losses.py:27-58), differentiable
    in ``rate`` and ``dispersion``: ``backward()`` delivers the closed-form gradients of ``nb_nll_grad``."""
    return _NegativeBinomialNLL.apply(y, rate, dispersion, mask, eps, backend)


def _heads_torch(hidden, w_mu, b_mu, w_sigma, b_sigma, tail, hist, late, floor, min_sigma):
    """``TimesNet._rate_dispersion``'s torch composition (models/timesnet.py:2063-2102 of the reference) with its
    check left on the device: ``(rate, dispersion, bad)``, ``bad`` one int32 with bit 0 / 1 set when a rate /
    dispersion is not finite and > 0 (the word of ``runtime.head_forward``)."""
    steps = hidden.shape[1]
    last = tail
    if hist < steps:                                            # short windows: repeat the last step
        last = torch.cat([last, last[:, -1:, :].expand(-1, steps - hist, -1)], dim=1)
    pre = F.linear(hidden, w_mu, b_mu) + last.to(hidden.dtype)
    if late is not None:
        pre = pre + late.to(pre.dtype)
    rate = F.softplus(pre, beta=1.0, threshold=20) + 1e-6
    spread = F.softplus(F.linear(hidden, w_sigma, b_sigma), beta=1.0, threshold=20)
    low = min_sigma if floor is None else floor.to(device=spread.device, dtype=spread.dtype).reshape(1, 1, -1)
    dispersion = spread + low + 1e-6
    wrong = [(~(torch.isfinite(v) & (v > 0))).any().to(torch.int32) for v in (rate.detach(), dispersion.detach())]
    return rate, dispersion, (wrong[0] | (wrong[1] << 1)).reshape(1)


def head_nll(hidden: torch.Tensor, w_mu: torch.Tensor, b_mu: torch.Tensor, w_sigma: torch.Tensor,
             b_sigma: torch.Tensor, tail: torch.Tensor, hist: int, y: torch.Tensor,
             mask: torch.Tensor | None = None, late: torch.Tensor | None = None, floor: torch.Tensor | None = None,
             min_sigma: float = 1e-3):
    """The rate / dispersion heads on ``hidden [B, S, D]`` (``TimesNet.head_inputs``) and their negative-binomial loss
    against ``y [B, S, N]``: ``(loss, bad)``.  ``loss.backward()`` leaves gradients in the four head tensors (and in
    ``hidden`` / ``late`` when they require grad).  On fp32 ROCm tensors with d_model a multiple of 4 up to 512 it is
    three kernels forward (``ftn_head_fit_forward``, ``ftn_nb_nll_grad``) and ``ftn_head_backward`` backward
    (``_last_head_backend == "hip"``); otherwise the torch composition with the loss node.  ``bad`` is the device word
    of ``runtime.head_forward``; nothing synchronises."""
    if hidden.dim() != 3 or y.dim() != 3 or y.shape[:2] != hidden.shape[:2] or y.shape[2] != w_mu.shape[0]:
        raise ValueError(f"head_nll: hidden {tuple(hidden.shape)}, y {tuple(y.shape)} and w_mu {tuple(w_mu.shape)} do "
                         "not fit [B, S, D], [B, S, N] and [N, D]")
    if not 1 <= int(hist) <= hidden.shape[1] or tuple(tail.shape) != (hidden.shape[0], int(hist), w_mu.shape[0]):
        raise ValueError(f"head_nll: tail {tuple(tail.shape)} is not [B, hist = {hist}, N] with 1 <= hist <= S")
    global _last_head_backend
    params = (w_mu, b_mu, w_sigma, b_sigma)
    D = hidden.shape[2]
    if (hidden.is_cuda and D % 4 == 0 and D <= 512 and hidden.numel() > 0
            and all(t.is_cuda and t.dtype == torch.float32 for t in (hidden, y, tail) + params)
            and all(t.is_contiguous() and t.data_ptr() % 16 == 0 for t in (w_mu, w_sigma))):
        _last_head_backend = "hip"
        return _HeadNLL.apply(hidden, w_mu, b_mu, w_sigma, b_sigma, tail, int(hist), y, mask, late, floor,
                              float(min_sigma))
    _last_head_backend = "torch"
    rate, dispersion, bad = _heads_torch(hidden, w_mu, b_mu, w_sigma, b_sigma, tail, int(hist), late, floor,
                                         float(min_sigma))
    return negative_binomial_nll(y, rate, dispersion, mask), bad


class _HeadNLL(torch.autograd.Function):
    """Heads plus loss on the device: ``ftn_head_fit_forward`` (rate, dispersion and the two sigmoids) and
    ``ftn_nb_nll_grad`` (raw derivatives, the loss and the scale word) forward, ``ftn_head_backward`` backward."""

    @staticmethod
    def forward(ctx, hidden, w_mu, b_mu, w_sigma, b_sigma, tail, hist, y, mask, late, floor, min_sigma):
        from . import runtime as rt

        hid = hidden.detach().contiguous()
        dev = hid.device
        tail = tail.detach()
        if tail.stride(2) != 1 or tail.stride(1) != tail.shape[2]:
            tail = tail.contiguous()
        late_c = None if late is None else late.detach().to(device=dev, dtype=torch.float32).contiguous()
        floor_c = None if floor is None else floor.detach().to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
        rate, disp, sig_mu, sig_sg, bad = rt.head_fit_forward(
            hid, w_mu.detach(), b_mu.detach().contiguous(), w_sigma.detach(), b_sigma.detach().contiguous(), tail, hist,
            late_c, floor_c, min_sigma)
        words, g_rate, g_disp = rt.nb_nll_grad(_rows(y.detach()), rate, disp, _full_mask(mask, rate), scaled=False)
        ctx.save_for_backward(hid, w_mu.detach(), w_sigma.detach(), g_rate, g_disp, sig_mu, sig_sg, words)
        ctx.late_shape = None if late is None else tuple(late.shape)
        ctx.mark_non_differentiable(bad)
        return words[0].clone(), bad

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss, _grad_bad):
        from . import runtime as rt

        hid, w_mu, w_sigma, g_rate, g_disp, sig_mu, sig_sg, words = ctx.saved_tensors
        scale = (words[1:2] * grad_loss).contiguous()           # the device word times the incoming gradient
        dw_mu, db_mu, dw_sg, db_sg, d_hidden = rt.head_backward(hid, g_rate, g_disp, sig_mu, sig_sg, scale, w_mu,
                                                                w_sigma, want_hidden=ctx.needs_input_grad[0])
        d_late = None
        if ctx.late_shape is not None and ctx.needs_input_grad[9]:
            d_late = g_rate * sig_mu * scale                    # G_mu itself
            if ctx.late_shape[0] == 1 and d_late.shape[0] > 1:
                d_late = d_late.sum(0, keepdim=True)
            d_late = d_late.reshape(ctx.late_shape)
        return d_hidden, dw_mu, db_mu, dw_sg, db_sg, None, None, None, None, d_late, None, None


def refit_heads(model, batches, epochs: int = 1, lr: float = 1e-3, use_loss_mask: bool = False, optimizer=None):
    """Refit ``mu_head`` and ``sigma_head`` of a ``TimesNet`` on new data, everything else frozen: for every batch
    tuple of ``batches`` (a list, or ``windows.DeviceWindows``; the tuples of ``score.eval_metrics``)
    ``model.head_inputs`` -> ``head_nll`` -> ``backward()`` -> a step of ``optimizer`` (default: Adam with ``lr`` over
    the four head tensors).  The per-step losses stay on the device until the end: one synchronisation, which also
    reads the heads' ``bad`` words and raises the reference's RuntimeError if a rate or dispersion was not finite and
    > 0.  Returns the losses, fp32 ``[epochs * batches]`` on the host.  The model is left in the mode and with the
    ``requires_grad`` flags it came with."""
    from .score import _unpack_batch

    heads = [model.mu_head.weight, model.mu_head.bias, model.sigma_head.weight, model.sigma_head.bias]
    dev = heads[0].device
    flags = [(p, p.requires_grad) for p in model.parameters()]
    was_training = model.training
    losses, bads = [], []
    try:
        for p, _ in flags:
            p.requires_grad_(False)
        for p in heads:
            p.requires_grad_(True)
        opt = optimizer if optimizer is not None else torch.optim.Adam(heads, lr=lr)
        model.eval()
        for _ in range(int(epochs)):
            for batch in batches:
                xb, yb, mask, x_mark, _, static, ids = _unpack_batch(batch)
                move = lambda t: None if t is None else t.to(dev, non_blocking=True)
                hidden, tail, hist, late, floor = model.head_inputs(
                    move(xb), move(x_mark), move(static),
                    None if ids is None else ids.to(device=dev, dtype=torch.long, non_blocking=True))
                yb = move(yb)[:, :hidden.shape[1], :]
                if use_loss_mask and mask is None:
                    raise ValueError("refit_heads: use_loss_mask needs a mask in every batch")
                base = (move(mask)[:, :hidden.shape[1], :] > 0.0) if use_loss_mask else None
                opt.zero_grad(set_to_none=True)
                with torch.enable_grad():
                    loss, bad = head_nll(hidden, *heads, tail, hist, yb, base, late, floor, model.min_sigma)
                loss.backward()
                opt.step()
                losses.append(loss.detach())
                bads.append(bad)
    finally:
        for p, flag in flags:
            p.requires_grad_(flag)
        model.train(was_training)
    if not losses:
        raise ValueError("refit_heads: no batches")
    out, flag = torch.stack(losses), torch.cat(bads)
    host = torch.cat([out, flag.to(out.dtype)]).cpu()           # the one synchronisation
    seen = 0
    for v in host[len(losses):].tolist():
        seen |= int(v)
    for bit, name in ((1, "rate"), (2, "dispersion")):
        if seen & bit:
            raise RuntimeError(f"Predicted {name} must be finite and strictly positive")
    return host[:len(losses)]


# ------------------------------------------------------------------ the whole output side: time projection + heads
_last_timeproj_backend: Optional[str] = None  # which path the last ``time_projection`` took


class _TimeProjection(torch.autograd.Function):
    """``forecast_time_proj`` as one node: ``ftn_timeproj_forward`` (the bits of inference) forward,
    ``ftn_timeproj_backward`` backward.  ``seq`` is a constant: no ``d_seq`` is computed."""

    @staticmethod
    def forward(ctx, seq, wt, bt, rows=None):
        from . import runtime as rt

        seq = seq.detach().contiguous()
        ctx.save_for_backward(seq, *(() if rows is None else (rows,)))
        return rt.timeproj_forward(seq, wt.detach(), bt.detach(), rows=rows)

    @staticmethod
    @once_differentiable
    def backward(ctx, d_hidden):
        from . import runtime as rt

        seq, *rows = ctx.saved_tensors
        d_hidden = d_hidden.contiguous()
        if d_hidden.dtype != torch.float32 or d_hidden.data_ptr() % 16:     # (ftn_head_backward's own is neither)
            d_hidden = d_hidden.float().clone()
        dw, db = rt.timeproj_backward(seq, d_hidden, rows=rows[0] if rows else None)
        return None, dw if ctx.needs_input_grad[1] else None, db if ctx.needs_input_grad[2] else None, None


def time_projection(seq: torch.Tensor, wt: torch.Tensor, bt: torch.Tensor,
                    rows: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``hidden[b] = wt @ seq[b] + bt[:, None]``, ``[B, S, D]`` from ``seq [B, L, D]`` (``TimesNet.output_inputs``),
    ``wt [S, L]`` and ``bt [S]``, differentiable in ``wt`` and ``bt``.  ``wt`` / ``bt`` may be the row slices
    ``weight[-steps:]`` / ``bias[-steps:]`` of a taller projection: autograd scatters the gradient into the full
    parameter and the other rows get exact zeros.  On fp32 ROCm tensors with d_model a multiple of 4 up to 512 and a
    ``seq`` that does not require grad it is ``ftn_timeproj_forward`` (the bits of inference) with
    ``ftn_timeproj_backward`` as its backward (``_last_timeproj_backend == "hip"``); otherwise - CPU tensors, other
    dtypes, other widths, a ``seq`` that requires grad (no ``d_seq`` is computed here) - the torch composition
    ``torch.matmul(wt, seq) + bt.view(1, -1, 1)``.

    ``rows`` (an int64 vector beside ``seq``): ``seq`` is an item store ``[n_items, L, D]`` (``OutputCache.seq``) and
    the result ``[len(rows), S, D]`` is that of ``seq[rows]``, to the bit.  The device path reads the store in place
    (``ftn_timeproj_forward_rows`` / ``ftn_timeproj_backward_rows``, which clamp an index into the store); the torch
    composition is ``torch.matmul(wt, seq.index_select(0, rows)) + bt.view(1, -1, 1)``."""
    if rows is not None and (not isinstance(rows, torch.Tensor) or rows.dtype != torch.int64 or rows.dim() != 1
                             or rows.numel() < 1 or rows.device != seq.device):
        raise ValueError("time_projection: rows must be an int64 vector of at least one entry beside seq")
    if seq.dim() != 3 or wt.dim() != 2 or bt.dim() != 1 or wt.shape[1] != seq.shape[1] or bt.shape[0] != wt.shape[0]:
        raise ValueError(f"time_projection: seq {tuple(seq.shape)}, wt {tuple(wt.shape)} and bt {tuple(bt.shape)} do "
                         "not fit [B, L, D], [S, L] and [S]")
    global _last_timeproj_backend
    B, L, D = seq.shape
    S = wt.shape[0]
    if (seq.is_cuda and D % 4 == 0 and 4 <= D <= 512 and seq.numel() > 0 and S >= 1
            and all(t.is_cuda and t.dtype == torch.float32 and t.device == seq.device for t in (seq, wt, bt))
            and not (torch.is_grad_enabled() and seq.requires_grad)
            and (S == 1 or wt.stride(0) == L) and (L == 1 or wt.stride(1) == 1) and (S == 1 or bt.stride(0) == 1)
            and seq.data_ptr() % 16 == 0):
        _last_timeproj_backend = "hip"
        return _TimeProjection.apply(seq, wt, bt, None if rows is None else rows.contiguous())
    _last_timeproj_backend = "torch"
    return torch.matmul(wt, seq if rows is None else seq.index_select(0, rows)) + bt.view(1, -1, 1)


def output_nll(seq: torch.Tensor, wt: torch.Tensor, bt: torch.Tensor, w_mu: torch.Tensor, b_mu: torch.Tensor,
               w_sigma: torch.Tensor, b_sigma: torch.Tensor, tail: torch.Tensor, hist: int, y: torch.Tensor,
               mask: torch.Tensor | None = None, late: torch.Tensor | None = None, floor: torch.Tensor | None = None,
               min_sigma: float = 1e-3, rows: Optional[torch.Tensor] = None):
    """The whole output side on ``seq [B, L, D]`` (``TimesNet.output_inputs``): ``time_projection`` then ``head_nll``,
    ``(loss, bad)``.  ``loss.backward()`` leaves gradients in ``wt``, ``bt`` and the four head tensors; on the device
    path every one of them comes from ``ftn_head_backward`` (which also writes ``d_hidden``) and
    ``ftn_timeproj_backward``.  ``rows``: ``seq`` is an item store read through this list (``time_projection``); the
    other operands are the batch's."""
    hidden = time_projection(seq, wt, bt, rows)
    return head_nll(hidden, w_mu, b_mu, w_sigma, b_sigma, tail, hist, y, mask, late, floor, min_sigma)


_last_late_backend: Optional[str] = None      # which path the last ``late_bias`` took


class _LateBias(torch.autograd.Function):
    """The late-bias head as one node: ``ftn_late_fit_forward`` (the bits of inference) forward, ``ftn_late_backward``
    backward.  The series rows are constants: no gradient in them."""

    @staticmethod
    def forward(ctx, rows, gamma, beta, weight, bias, gate, eps, index):
        from . import runtime as rt

        ops = [t.detach().contiguous() for t in (rows, gamma, beta, weight, bias, gate)]
        ctx.save_for_backward(*ops, *(() if index is None else (index,)))
        ctx.eps, ctx.gate_shape = eps, tuple(gate.shape)
        return rt.late_fit_forward(*ops, eps, rows=index)

    @staticmethod
    @once_differentiable
    def backward(ctx, d_late):
        from . import runtime as rt

        rows, gamma, beta, weight, bias, gate, *index = ctx.saved_tensors
        d_pre = d_late.contiguous()
        if d_pre.dtype != torch.float32:
            d_pre = d_pre.float()
        dg, dbt, dw, db, dgate = rt.late_backward(d_pre, rows, gamma, beta, weight, bias, gate, ctx.eps,
                                                  rows=index[0] if index else None)
        need = ctx.needs_input_grad
        return (None, dg if need[1] else None, dbt if need[2] else None, dw if need[3] else None,
                db if need[4] else None, dgate.reshape(ctx.gate_shape) if need[5] else None, None, None)


def late_bias(rows: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor,
              gate: torch.Tensor, eps: float, index: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The gated late bias ``gate * (weight LayerNorm(rows) + bias)^T`` of the frozen series rows ``rows [Bc, N, ctx]``
    (``TimesNet.late_rows``): ``[Bc, S, N]``, differentiable in ``gamma`` / ``beta`` ``[ctx]`` (``late_bias_norm``),
    ``weight [S, ctx]`` / ``bias [S]`` (``late_bias_head``) and ``gate`` (``late_bias_gate``, ``[1, S, 1]`` or
    ``[S]``) - the ``late=`` of ``head_nll`` / ``output_nll``.  ``index`` (an int64 vector beside ``rows``): ``rows``
    is an item store ``[n_items, ctx]`` and the result ``[len(index), S, 1]`` is that of ``rows[index][:, None]``, to
    the bit.  On fp32 ROCm tensors with ``ctx <= 256`` and rows that do not require grad it is
    ``ftn_late_fit_forward`` (the bits of the model's own late bias) with ``ftn_late_backward`` as its backward
    (``_last_late_backend == "hip"``; the kernels clamp an index into the store); otherwise the torch composition."""
    if index is not None and (not isinstance(index, torch.Tensor) or index.dtype != torch.int64 or index.dim() != 1
                              or index.numel() < 1 or index.device != rows.device):
        raise ValueError("late_bias: index must be an int64 vector of at least one entry beside rows")
    if rows.dim() != (3 if index is None else 2) or rows.numel() < 1:
        raise ValueError(f"late_bias: rows {tuple(rows.shape)} are not " +
                         ("[Bc, N, ctx]" if index is None else "an item store [n_items, ctx]"))
    ctx_w = rows.shape[-1]
    if (weight.dim() != 2 or weight.shape[1] != ctx_w or gamma.shape != (ctx_w,) or beta.shape != (ctx_w,)
            or bias.shape != (weight.shape[0],) or gate.numel() != weight.shape[0]
            or tuple(gate.shape) not in ((weight.shape[0],), (1, weight.shape[0], 1))):
        raise ValueError(f"late_bias: gamma {tuple(gamma.shape)}, beta {tuple(beta.shape)}, weight {tuple(weight.shape)}, "
                         f"bias {tuple(bias.shape)} and gate {tuple(gate.shape)} do not fit [ctx = {ctx_w}], [ctx], "
                         "[S, ctx], [S] and [1, S, 1]")
    global _last_late_backend
    ops = (rows, gamma, beta, weight, bias, gate)
    if (rows.is_cuda and ctx_w <= 256 and all(t.is_cuda and t.dtype == torch.float32 and t.device == rows.device
                                              for t in ops)
            and not (torch.is_grad_enabled() and rows.requires_grad)):
        _last_late_backend = "hip"
        return _LateBias.apply(rows, gamma, beta, weight, bias, gate, float(eps),
                               None if index is None else index.contiguous())
    _last_late_backend = "torch"
    r = rows if index is None else rows.index_select(0, index).unsqueeze(1)
    lb = F.linear(F.layer_norm(r, (ctx_w,), gamma, beta, float(eps)), weight, bias)
    return gate.reshape(1, -1, 1) * lb.transpose(1, 2)


_late_bias_node = late_bias                    # (``late_bias`` is also the name of the refit loops' switch)


def _late_params(model):
    """The five late-bias tensors in the order a refit lists them, or a ValueError for a model without the head."""
    norm, head, gate = (getattr(model, n, None) for n in ("late_bias_norm", "late_bias_head", "late_bias_gate"))
    if (norm is None or head is None or not isinstance(gate, torch.nn.Parameter)
            or getattr(norm, "weight", None) is None or getattr(norm, "bias", None) is None):
        raise ValueError("late_bias=True: the model has no late-bias head (use_late_bias_head with ids or statics, "
                         "built by a first forward)")
    return [norm.weight, norm.bias, head.weight, head.bias, gate]


def refit_output(model, batches, epochs: int = 1, lr: float = 1e-3, use_loss_mask: bool = False, optimizer=None,
                 grad_clip: Optional[float] = None, late_bias: bool = False):
    """``refit_heads`` over the whole output side of a ``TimesNet``: ``forecast_time_proj`` (its last
    ``model._out_steps`` rows are what a step reads; the other rows of a recursive model get zero gradients),
    ``mu_head`` and ``sigma_head``, everything else frozen.  Per batch ``model.output_inputs`` -> ``output_nll`` ->
    ``backward()`` -> (with ``grad_clip``, the reference's ``clip_grad_norm_`` over the six tensors, train.py:1513-1515)
    -> a step of ``optimizer`` (default: Adam with ``lr`` over the six tensors).  Losses and ``bad`` words stay on
    the device until the one synchronisation at the end, which raises the reference's RuntimeError if a rate or
    dispersion was not finite and > 0.  Returns the losses, fp32 ``[epochs * batches]`` on the host; mode and
    ``requires_grad`` flags come back as they were.

    ``late_bias=True``: the late-bias head moves too - eleven tensors, the six in their order, then
    ``late_bias_norm.weight`` / ``.bias``, ``late_bias_head.weight`` / ``.bias`` and ``late_bias_gate``; per batch the
    frozen series rows ``model.late_rows`` go through ``late_bias`` into the ``late=`` of ``output_nll``, and
    ``grad_clip`` is the global norm over all eleven.  A model without the head is a ValueError."""
    from .score import _unpack_batch

    proj = model.forecast_time_proj
    params = [model.mu_head.weight, model.mu_head.bias, model.sigma_head.weight, model.sigma_head.bias,
              proj.weight, proj.bias]
    if late_bias:
        if getattr(model, "late_bias_head", None) is None and getattr(model, "use_late_bias_head", False):
            first = next(iter(batches), None)                  # the head is built by the first forward
            if first is not None:
                xb, _, _, x_mark, _, static, ids = _unpack_batch(first)
                dev0 = params[0].device
                mv = lambda t: None if t is None else t.to(dev0)
                model.late_rows(mv(xb), mv(x_mark), mv(static),
                                None if ids is None else ids.to(device=dev0, dtype=torch.long))
        late_ps = _late_params(model)
        params = params + late_ps
    dev = params[0].device
    flags = [(p, p.requires_grad) for p in model.parameters()]
    was_training = model.training
    losses, bads = [], []
    try:
        for p, _ in flags:
            p.requires_grad_(False)
        for p in params:
            p.requires_grad_(True)
        opt = optimizer if optimizer is not None else torch.optim.Adam(params, lr=lr)
        model.eval()
        steps = int(model._out_steps)
        for _ in range(int(epochs)):
            for batch in batches:
                xb, yb, mask, x_mark, _, static, ids = _unpack_batch(batch)
                move = lambda t: None if t is None else t.to(dev, non_blocking=True)
                seq, tail, hist, late, floor = model.output_inputs(
                    move(xb), move(x_mark), move(static),
                    None if ids is None else ids.to(device=dev, dtype=torch.long, non_blocking=True))
                yb = move(yb)[:, :steps, :]
                if use_loss_mask and mask is None:
                    raise ValueError("refit_output: use_loss_mask needs a mask in every batch")
                base = (move(mask)[:, :steps, :] > 0.0) if use_loss_mask else None
                if late_bias:
                    srows = model.late_rows(
                        move(xb), move(x_mark), move(static),
                        None if ids is None else ids.to(device=dev, dtype=torch.long, non_blocking=True))
                opt.zero_grad(set_to_none=True)
                with torch.enable_grad():
                    if late_bias:
                        late = _late_bias_node(srows, *late_ps, model.late_bias_norm.eps)
                    loss, bad = output_nll(seq, proj.weight[-steps:], proj.bias[-steps:], *params[:4], tail, hist, yb,
                                           base, late, floor, model.min_sigma)
                loss.backward()
                if grad_clip is not None:
                    torch.nn.utils.clip_grad_norm_(params, float(grad_clip))
                opt.step()
                losses.append(loss.detach())
                bads.append(bad)
    finally:
        for p, flag in flags:
            p.requires_grad_(flag)
        model.train(was_training)
    if not losses:
        raise ValueError("refit_output: no batches")
    return _losses_or_raise(losses, bads)


def _losses_or_raise(losses, bads) -> torch.Tensor:
    """The one synchronisation of a refit loop: the losses on the host, after the reference's RuntimeError if any
    ``bad`` word has a bit set."""
    out, flag = torch.stack(losses), torch.cat(bads)
    host = torch.cat([out, flag.to(out.dtype)]).cpu()
    seen = 0
    for v in host[len(losses):].tolist():
        seen |= int(v)
    for bit, name in ((1, "rate"), (2, "dispersion")):
        if seen & bit:
            raise RuntimeError(f"Predicted {name} must be finite and strictly positive")
    return host[:len(losses)]


# ------------------------------------------------------------------ the refit step on the device: clip + AdamW, one graph
_last_optim_backend: Optional[str] = None     # which path the last ``DeviceAdamW`` update took


def _bump_versions(tensors) -> None:
    """What an in-place torch op does to a tensor's version counter, for tensors a kernel of ours wrote: caches keyed
    on ``models.timesnet._param_key`` (``series_slices``, the pack caches) then see the step."""
    for t in tensors:
        if not t.is_inference():
            torch.autograd.graph.increment_version(t)


class DeviceAdamW:
    """AdamW after a clip by the global gradient norm (torch's ``clip_grad_norm_`` then ``torch.optim.AdamW``) whose
    step count, learning rate, norm and decision to skip live on the device: ``ftn_refit_update``
    (``csrc/refit.hip``) on contiguous fp32 ROCm tensors (backend ``hip``), the same formulas in torch ops anywhere
    else (backend ``torch``); ``_last_optim_backend`` says which ran.  Up to 8 parameter tensors.  Nothing is read on
    the host, so a step can be captured in a HIP graph.

    The update is skipped - parameters, moments and the step count keep every bit - when a ``skip`` word is non-zero
    (a head's ``bad`` word, a block's f16x2 range word), the gradient norm is not finite or the loss word is not
    finite.  Every call, skipped or not, writes ``(loss, norm before clipping, lr, flags)`` to a ring of
    ``log_steps`` rows; ``history()`` returns the rows since its last call.  Flags: 1 rate bad, 2 dispersion bad,
    4 range word set, 8 norm or loss not finite.

    ``zero_grad`` / ``step`` read ``p.grad`` as a torch optimizer does (``refit_output(..., optimizer=...)``);
    ``step_on`` takes caller-owned gradient buffers."""

    _max_tensors = 8
    _entry = "refit_update"                     # the ``runtime`` function of the device path

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 max_norm: Optional[float] = None, log_steps: int = 4096, backend: Optional[str] = None):
        self.params = list(params)
        if not 1 <= len(self.params) <= self._max_tensors:
            raise ValueError(f"{type(self).__name__}: {len(self.params)} parameter tensors (1..{self._max_tensors})")
        for p in self.params:
            if not isinstance(p, torch.Tensor) or not p.is_floating_point() or p.numel() < 1:
                raise ValueError("DeviceAdamW: parameters must be floating-point tensors that are not empty")
        if len({p.device for p in self.params}) != 1:
            raise ValueError("DeviceAdamW: parameters must be on one device")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"DeviceAdamW: betas={tuple(betas)} are not inside [0, 1)")
        if not (lr >= 0.0 and eps >= 0.0 and weight_decay >= 0.0):
            raise ValueError(f"DeviceAdamW: lr={lr}, eps={eps} and weight_decay={weight_decay} must be >= 0")
        if int(log_steps) < 1:
            raise ValueError(f"DeviceAdamW: log_steps={log_steps} must be >= 1")
        if backend not in (None, "hip", "torch"):
            raise ValueError(f"DeviceAdamW: backend {backend!r} is not 'hip', 'torch' or None")
        self.betas, self.eps, self.weight_decay = (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        self.max_norm = None if max_norm is None or float(max_norm) <= 0.0 else float(max_norm)
        self.backend = backend
        dev = self.device = self.params[0].device
        self.exp_avg = [torch.zeros_like(p, memory_format=torch.contiguous_format) for p in self.params]
        self.exp_avg_sq = [torch.zeros_like(p, memory_format=torch.contiguous_format) for p in self.params]
        self._lr = torch.full((1,), float(lr), dtype=torch.float32, device=dev)
        self._state = torch.zeros(2, dtype=torch.int32, device=dev)      # [t, calls]
        self._log = torch.zeros(int(log_steps), 4, dtype=torch.float32, device=dev)
        self._calls = 0                                                   # the host's count of calls
        self._read = 0                                                    # calls ``history()`` has returned

    # ---- the torch optimizer's surface ----
    def zero_grad(self, set_to_none: bool = True) -> None:
        for p in self.params:
            if set_to_none:
                p.grad = None
            elif p.grad is not None:
                p.grad.detach_().zero_()

    def step(self, loss: Optional[torch.Tensor] = None, skip=()) -> None:
        """The update from ``p.grad`` of every parameter that has one."""
        idx = [i for i, p in enumerate(self.params) if p.grad is not None]
        if not idx:
            raise ValueError("DeviceAdamW.step: no parameter has a gradient")
        self._update(idx, [self.params[i].grad for i in idx], loss, skip)

    def step_on(self, grads, loss: Optional[torch.Tensor] = None, skip=()) -> None:
        """The update from ``grads`` (one tensor per parameter, read only).  ``loss``: an optional 0-dim or one-element
        fp32 tensor on the device, logged and checked for finiteness.  ``skip``: int32 device words; an entry may be
        ``(word, "range")`` to mark a block's range word (flag 4), a bare word is a head's ``bad`` word."""
        grads = list(grads)
        if len(grads) != len(self.params):
            raise ValueError(f"DeviceAdamW.step_on: {len(grads)} gradients for {len(self.params)} parameters")
        self._update(list(range(len(grads))), grads, loss, skip)

    def set_lr(self, value: float) -> None:
        """An asynchronous fill of the device word: the next update, a replayed one too, uses it."""
        self._lr.fill_(float(value))

    def note_replay(self, calls: int = 1) -> None:
        """What a replay of a captured ``step_on`` leaves to the host: the call count ``history()`` goes by and the
        parameters' version counters."""
        self._calls += int(calls)
        _bump_versions(self.params)

    def history(self) -> torch.Tensor:
        """The log rows ``[calls, 4]`` = (loss, norm before clipping, lr, flags) of the calls since the last
        ``history()`` (the last ``log_steps`` of them at most), on the host: one synchronisation."""
        cap = self._log.shape[0]
        first = max(self._read, self._calls - cap)
        rows = self._log.cpu()
        self._read = self._calls
        return rows[[k % cap for k in range(first, self._calls)]].reshape(-1, 4)

    def state_dict(self) -> dict:
        return {"t": int(self._state[0].item()), "exp_avg": [m.detach().clone() for m in self.exp_avg],
                "exp_avg_sq": [v.detach().clone() for v in self.exp_avg_sq]}

    def load_state_dict(self, state: dict) -> None:
        if len(state["exp_avg"]) != len(self.params) or len(state["exp_avg_sq"]) != len(self.params):
            raise ValueError("DeviceAdamW.load_state_dict: the state is for another number of parameters")
        for dst, src in zip(self.exp_avg + self.exp_avg_sq, list(state["exp_avg"]) + list(state["exp_avg_sq"])):
            if tuple(dst.shape) != tuple(src.shape):
                raise ValueError("DeviceAdamW.load_state_dict: a moment has another shape")
        with torch.no_grad():
            for dst, src in zip(self.exp_avg + self.exp_avg_sq, list(state["exp_avg"]) + list(state["exp_avg_sq"])):
                dst.copy_(src)
            self._state[0:1].fill_(int(state["t"]))

    # ---- the update ----
    def _update(self, idx, grads, loss, skip) -> None:
        global _last_optim_backend
        from .range_guard import _capturing

        ps = [self.params[i] for i in idx]
        ms, vs = [self.exp_avg[i] for i in idx], [self.exp_avg_sq[i] for i in idx]
        for p, g in zip(ps, grads):
            if not isinstance(g, torch.Tensor) or tuple(g.shape) != tuple(p.shape) or g.device != p.device:
                raise ValueError("DeviceAdamW: a gradient does not have its parameter's shape and device")
        words, range_mask = [], 0
        for k, w in enumerate(skip):
            if isinstance(w, tuple):
                if len(w) != 2 or w[1] != "range":
                    raise ValueError("DeviceAdamW: a skip entry is a word or (word, 'range')")
                w, range_mask = w[0], range_mask | 1 << k
            if not isinstance(w, torch.Tensor) or w.dtype != torch.int32 or w.numel() != 1 or w.device != self.device:
                raise ValueError("DeviceAdamW: a skip word must be one int32 beside the parameters")
            words.append(w)
        if len(words) > 8:
            raise ValueError(f"DeviceAdamW: {len(words)} skip words (at most 8)")
        if loss is not None and (not isinstance(loss, torch.Tensor) or loss.numel() != 1
                                 or loss.device != self.device or not loss.is_floating_point()):
            raise ValueError("DeviceAdamW: loss must be one floating-point word beside the parameters")
        eligible = (self.device.type == "cuda"
                    and all(t.dtype == torch.float32 for t in ps + list(grads))
                    and all(p.is_contiguous() for p in ps)
                    and (loss is None or loss.dtype == torch.float32))
        if _use_hip("DeviceAdamW", self.backend, eligible, "contiguous fp32 parameters and fp32 gradients on a ROCm device"):
            from . import runtime as rt

            getattr(rt, self._entry)([p.detach() for p in ps], [g.detach().contiguous() for g in grads], ms, vs,
                                     self._lr, self._state, self.betas, self.eps, self.weight_decay, self.max_norm,
                                     words, range_mask, None if loss is None else loss.detach().reshape(1), self._log)
            _last_optim_backend = "hip"
            if not _capturing():
                _bump_versions(ps)
        else:
            with torch.no_grad():
                self._update_torch(ps, [g.detach() for g in grads], ms, vs, loss, words, range_mask)
            _last_optim_backend = "torch"
        if not _capturing():
            self._calls += 1

    def _update_torch(self, ps, grads, ms, vs, loss, words, range_mask) -> None:
        """``ftn_refit_update`` in torch ops: fp64 for the sum of squares, the clip coefficient, the decay factor and
        the bias corrections, each rounded once to the parameter's dtype; element arithmetic in that dtype.  The
        decision is a device word and the update a ``torch.where``: nothing is read on the host."""
        dev = self.device
        f64 = dict(dtype=torch.float64, device=dev)
        total = torch.zeros((), **f64)
        for g in grads:
            total = total + g.double().square().sum()
        norm = total.sqrt()
        flags = torch.zeros((), dtype=torch.int32, device=dev)
        for k, w in enumerate(words):
            w = w.reshape(())
            if range_mask >> k & 1:
                flags = flags | (w != 0).to(torch.int32) * 4
            else:
                flags = flags | (w & 3) | ((w & ~3) != 0).to(torch.int32) * 8
        loss_w = torch.zeros((), dtype=torch.float32, device=dev) if loss is None else loss.detach().reshape(()).float()
        flags = flags | (~(torch.isfinite(norm) & torch.isfinite(loss_w))).to(torch.int32) * 8
        keep = flags == 0
        one = torch.ones((), **f64)
        c = one if self.max_norm is None else torch.clamp(self.max_norm / (norm + 1e-6), max=1.0)
        c = torch.where(torch.isnan(c), one, c)
        t1 = (self._state[0] + 1).double()
        b1, b2 = self.betas
        bc1, bc2 = 1.0 - torch.pow(torch.tensor(b1, **f64), t1), 1.0 - torch.pow(torch.tensor(b2, **f64), t1)
        lr = self._lr[0]
        decay, step, rs = 1.0 - lr.double() * self.weight_decay, lr.double() / bc1, bc2.sqrt()
        for p, g, m, v in zip(ps, grads, ms, vs):
            dt = p.dtype
            gc = c.to(dt) * g.to(dt)
            m_new = b1 * m + (1.0 - b1) * gc
            v_new = b2 * v + ((1.0 - b2) * gc) * gc
            p_new = p * decay.to(dt) - step.to(dt) * (m_new / (v_new.sqrt() / rs.to(dt) + self.eps))
            p.copy_(torch.where(keep, p_new, p))
            m.copy_(torch.where(keep, m_new, m))
            v.copy_(torch.where(keep, v_new, v))
        row = torch.stack([loss_w, norm.float(), lr, flags.float()])
        self._log.index_copy_(0, (self._state[1:2] % self._log.shape[0]).long(), row.reshape(1, 4))
        self._state += torch.stack([keep.to(torch.int32), torch.ones((), dtype=torch.int32, device=dev)])


class DeviceAdamWList(DeviceAdamW):
    """``DeviceAdamW`` for 1 to 32 parameter tensors: one clip-and-AdamW step over all of them - one global norm, one
    decision, one ``t``, one log row - through ``ftn_refit_update_list`` (``csrc/refit.hip``), which walks the list in
    records of 8 that share the norm.  Up to 8 tensors it is ``DeviceAdamW`` bit for bit; the torch backend is
    ``DeviceAdamW``'s, which takes any count."""

    _max_tensors = 32
    _entry = "refit_update_list"


def _refit_params(model):
    proj = model.forecast_time_proj
    return [model.mu_head.weight, model.mu_head.bias, model.sigma_head.weight, model.sigma_head.bias,
            proj.weight, proj.bias]


class GraphedRefitStep:
    """One step of ``refit_output`` - backbone forward, time projection, heads, loss, both backwards, clip and AdamW -
    captured once and replayed with a single graph launch: ``step(batch)`` copies the batch into the captured buffers
    (``.inputs``: ``x, y, mask, x_mark, static, ids``, None where the captured batch had none; ``DeviceWindows`` may
    write into them directly) and replays.  Nothing is read on the host.  The launches and their operands are the
    ones ``_TimeProjection`` and ``_HeadNLL`` make, so a step's gradients (``.grads``, in ``refit_output``'s parameter
    order) have the bits of the eager ``output_nll`` backward; the time projection's gradient goes into the last
    ``steps`` rows of a zeroed full-size buffer, so the other rows of a recursive model only decay.  The update is
    ``optimizer.step_on`` with the heads' ``bad`` word and the blocks' f16x2 range words as skip words: a replay that
    trips one leaves parameters and moments as they were and logs the flag.  Shapes and which optional pieces exist
    are frozen at capture; a batch that differs is a ValueError."""

    def __init__(self, model, batch, optimizer: DeviceAdamW, use_loss_mask: bool = False, warmup: int = 2):
        from .score import _unpack_batch

        if not isinstance(optimizer, DeviceAdamW):
            raise ValueError("GraphedRefitStep needs a fit.DeviceAdamW")
        params = _refit_params(model)
        if len(optimizer.params) != 6 or any(a is not b for a, b in zip(optimizer.params, params)):
            raise ValueError("GraphedRefitStep: the optimizer must hold mu_head, sigma_head and forecast_time_proj "
                             "(weight, bias each, in that order)")
        dev = params[0].device
        if dev.type != "cuda" or any(p.dtype != torch.float32 or not p.is_contiguous() for p in params):
            raise ValueError("GraphedRefitStep needs a model with contiguous fp32 parameters on a ROCm device")
        xb, yb, mask, x_mark, _, static, ids = _unpack_batch(batch)
        if use_loss_mask and mask is None:
            raise ValueError("GraphedRefitStep: use_loss_mask needs a mask in the batch")
        self.model, self.optimizer, self.device = model, optimizer, dev
        self.use_loss_mask = bool(use_loss_mask)
        self.steps = int(model._out_steps)
        own = lambda t, dtype=None: None if t is None else t.to(device=dev, dtype=dtype).clone()
        self._in = (own(xb), own(yb), own(mask) if use_loss_mask else None, own(x_mark), own(static),
                    own(ids, torch.long))
        proj = model.forecast_time_proj
        self._gw, self._gb = torch.zeros_like(proj.weight), torch.zeros_like(proj.bias)   # rows before -steps stay 0
        if model.training:
            raise ValueError("GraphedRefitStep: put the model in eval mode first (refit_output_graphed does)")
        # warm-up on a side stream: lazy builds, packing, the allocator.  The update goes to copies of the parameters
        # and a throw-away optimizer, so neither the model nor the moments move before the first step.
        spare = DeviceAdamW([p.detach().clone() for p in params], backend="hip")
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side), torch.no_grad():
            for _ in range(max(1, int(warmup))):
                self._enqueue(spare)
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        # a model first called on the host and then moved remembers its id row there and copies it per call, which no
        # capture takes; given ids are checked with a host read unless the checks are deferred (graph.GraphedForward)
        remembered = getattr(model, "_series_id_reference", None)
        if isinstance(remembered, torch.Tensor) and remembered.device != dev:
            model._series_id_reference = remembered.to(dev)
        self.graph = torch.cuda.CUDAGraph()
        deferred = getattr(model, "_defer_checks", False)
        model._defer_checks = True
        try:
            with torch.no_grad(), torch.cuda.graph(self.graph):
                self.loss, self.bad, self.grads, self._keep = self._enqueue(optimizer)
        finally:
            model._defer_checks = deferred
        self.range_words = [b._range_dev_flag for b in model.blocks if getattr(b, "_range_dev_flag", None) is not None]
        # addresses the captured launches have baked in (as graph.GraphedForward)
        self._packs = [m._pack for m in model.modules() if getattr(m, "_pack", None) is not None]

    def _enqueue(self, optimizer: DeviceAdamW):
        """The step's launches on the current stream, in ``refit_output``'s order."""
        from . import runtime as rt

        model, steps = self.model, self.steps
        x, y, mask, x_mark, static, ids = self._in
        w_mu, b_mu, w_sg, b_sg, pw, pb = (p.detach() for p in _refit_params(model))
        seq, tail, hist, late, floor = model.output_inputs(x, x_mark, static, ids)
        ranges = [b._range_dev_flag for b in model.blocks if getattr(b, "_range_dev_flag", None) is not None] \
            if torch.cuda.is_current_stream_capturing() else []
        seq = seq.detach().contiguous()
        D = seq.shape[2]
        if not (D % 4 == 0 and 4 <= D <= 512 and seq.dtype == torch.float32 and seq.data_ptr() % 16 == 0
                and w_mu.data_ptr() % 16 == 0 and w_sg.data_ptr() % 16 == 0):
            raise ValueError("GraphedRefitStep: the output side of this model does not take the HIP path (fp32, "
                             "d_model a multiple of 4 up to 512, weights on the 16-byte grid)")
        hidden = rt.timeproj_forward(seq, pw[-steps:], pb[-steps:])
        tail = tail.detach()
        if tail.stride(2) != 1 or tail.stride(1) != tail.shape[2]:
            tail = tail.contiguous()
        late_c = None if late is None else late.detach().to(device=self.device, dtype=torch.float32).contiguous()
        floor_c = None if floor is None else floor.detach().to(device=self.device,
                                                               dtype=torch.float32).reshape(-1).contiguous()
        rate, disp, sig_mu, sig_sg, bad = rt.head_fit_forward(hidden, w_mu, b_mu.contiguous(), w_sg, b_sg.contiguous(),
                                                              tail, hist, late_c, floor_c, float(model.min_sigma))
        base = (mask[:, :steps, :] > 0.0) if self.use_loss_mask else None
        words, g_rate, g_disp = rt.nb_nll_grad(_rows(y[:, :steps, :]), rate, disp, _full_mask(base, rate),
                                               scaled=False)
        dw_mu, db_mu, dw_sg, db_sg, d_hidden = rt.head_backward(hidden, g_rate, g_disp, sig_mu, sig_sg,
                                                                words[1:2], w_mu, w_sg, want_hidden=True)
        rt.timeproj_backward(seq, d_hidden, dw=self._gw[-steps:], db=self._gb[-steps:])
        grads = [dw_mu, db_mu, dw_sg, db_sg, self._gw, self._gb]
        optimizer.step_on(grads, loss=words[0:1], skip=[bad] + [(w, "range") for w in ranges])
        keep = (seq, hidden, tail, late_c, floor_c, rate, disp, sig_mu, sig_sg, base, words, g_rate, g_disp, d_hidden)
        return words[0:1], bad, grads, keep

    @property
    def inputs(self):
        """The captured buffers ``(x, y, mask, x_mark, static, ids)``; writing into them saves ``step``'s copy."""
        return self._in

    def replay(self) -> torch.Tensor:
        """One replay on the buffers as they are; returns the loss word (overwritten by the next replay)."""
        self.graph.replay()
        self.optimizer.note_replay()
        return self.loss

    def _given(self, batch):
        """``batch`` as ``(name, captured buffer, given tensor)`` triples, and the first name that does not fit."""
        from .score import _unpack_batch

        xb, yb, mask, x_mark, _, static, ids = _unpack_batch(batch)
        given = (xb, yb, mask if self.use_loss_mask else None, x_mark, static, ids)
        triples = list(zip(("x", "y", "mask", "x_mark", "static", "ids"), self._in, given))
        odd = next((t for t in triples if (t[1] is None) != (t[2] is None)
                    or (t[1] is not None and tuple(t[1].shape) != tuple(t[2].shape))), None)
        return triples, odd

    def fits(self, batch) -> bool:
        """Whether ``batch`` has the captured shapes and optional pieces."""
        return self._given(batch)[1] is None

    def step(self, batch) -> torch.Tensor:
        """Copies ``batch`` into the captured buffers (a tensor that already is its buffer is left alone) and replays;
        returns the loss word."""
        triples, odd = self._given(batch)
        if odd is not None:
            name, dst, src = odd
            raise ValueError(f"GraphedRefitStep.step: {name} is {'absent' if src is None else tuple(src.shape)}, "
                             f"captured {'absent' if dst is None else tuple(dst.shape)}")
        for _, dst, src in triples:
            if dst is not None and src.data_ptr() != dst.data_ptr():
                dst.copy_(src, non_blocking=True)
        return self.replay()


_RANGE_MESSAGE = ("a value left the fp16 range of engine f16x2 inside a captured step; the steps it happened in were "
                  "skipped: set block.engine = 'bf16x3' on the model's blocks and refit")


def refit_output_graphed(model, batches, epochs: int = 1, lr=1e-3, weight_decay: float = 0.0,
                         grad_clip: Optional[float] = None, use_loss_mask: bool = False):
    """``refit_output``'s loop over a ``GraphedRefitStep`` with a ``DeviceAdamW``: one graph launch per batch, one
    synchronisation at the end.  ``lr``: a float, or one value per epoch (``DeviceAdamW.set_lr``).  A batch whose
    shapes differ from the first one's (a short last batch) takes the eager step of ``refit_output`` with the same
    optimizer.  Returns the losses, fp32 ``[epochs * batches]`` on the host, after the reference's RuntimeError if a
    logged step found a rate or dispersion not finite and > 0, and ``FloatingPointError`` if one left the fp16 range
    of engine f16x2 (those steps were skipped; set ``block.engine = "bf16x3"`` and refit).  Mode and
    ``requires_grad`` flags come back as they were."""
    from .score import _unpack_batch

    epochs = int(epochs)
    rates = [float(lr)] * epochs if isinstance(lr, (int, float)) else [float(v) for v in lr]
    if len(rates) != epochs:
        raise ValueError(f"refit_output_graphed: {len(rates)} learning rates for {epochs} epochs")
    params = _refit_params(model)
    dev = params[0].device
    flags = [(p, p.requires_grad) for p in model.parameters()]
    was_training = model.training
    losses = []
    try:
        for p, _ in flags:
            p.requires_grad_(False)
        for p in params:
            p.requires_grad_(True)
        model.eval()
        opt = DeviceAdamW(params, lr=rates[0] if rates else 1e-3, weight_decay=weight_decay, max_norm=grad_clip)
        step, steps = None, int(model._out_steps)
        for epoch in range(epochs):
            opt.set_lr(rates[epoch])
            for batch in batches:
                if step is None:
                    step = GraphedRefitStep(model, batch, opt, use_loss_mask=use_loss_mask)
                if step.fits(batch):
                    losses.append(step.step(batch).clone())
                    continue
                xb, yb, mask, x_mark, _, static, ids = _unpack_batch(batch)
                move = lambda t: None if t is None else t.to(dev, non_blocking=True)
                seq, tail, hist, late, floor = model.output_inputs(
                    move(xb), move(x_mark), move(static),
                    None if ids is None else ids.to(device=dev, dtype=torch.long, non_blocking=True))
                if use_loss_mask and mask is None:
                    raise ValueError("refit_output_graphed: use_loss_mask needs a mask in every batch")
                base = (move(mask)[:, :steps, :] > 0.0) if use_loss_mask else None
                opt.zero_grad(set_to_none=True)
                with torch.enable_grad():
                    proj = model.forecast_time_proj
                    loss, bad = output_nll(seq, proj.weight[-steps:], proj.bias[-steps:], *params[:4], tail, hist,
                                           move(yb)[:, :steps, :], base, late, floor, model.min_sigma)
                loss.backward()
                opt.step(loss=loss.detach(), skip=[bad])
                opt.zero_grad(set_to_none=True)
                losses.append(loss.detach().reshape(1))
    finally:
        for p, flag in flags:
            p.requires_grad_(flag)
        model.train(was_training)
    if not losses:
        raise ValueError("refit_output_graphed: no batches")
    host = torch.cat(losses).cpu()                               # the one synchronisation
    seen = 0
    for v in opt.history()[:, 3].tolist():
        seen |= int(v)
    for bit, name in ((1, "rate"), (2, "dispersion")):
        if seen & bit:
            raise RuntimeError(f"Predicted {name} must be finite and strictly positive")
    if seen & 4:
        raise FloatingPointError("refit_output_graphed: " + _RANGE_MESSAGE)
    return host


# ------------------------------------------------------------------ cached refit: the frozen backbone once per item
def _late_layout(model, windows) -> Optional[str]:
    """How the late bias of ``model`` lies over the items of ``windows``, from the host alone: ``"item"`` (the series
    layout hands statics or ids per item, so the series rows differ per item), ``"shared"`` (one ``[1, steps, N]``
    block) or None (no late-bias head, or no series rows to feed it)."""
    from torch import nn

    statics = windows._has_static and model.static_proj is not None
    if (model.late_bias_head is None or model.late_bias_norm is None
            or not isinstance(model.late_bias_gate, nn.Parameter) or not (statics or model._uses_ids())):
        return None
    per_item = windows.layout == "series" and (statics or (windows._has_ids and model._uses_ids()))
    return "item" if per_item else "shared"


class OutputCache:
    """What the output side of a frozen ``TimesNet`` reads, kept per item of a ``windows.DeviceWindows``: ``seq
    [n_items, L, D]`` (the block stack's output), ``tail [n_items, hist, N]``, ``y [n_items, steps, N]``, ``mask``
    (fp32 0/1, only with ``use_loss_mask``), ``late`` (``[n_items, steps, N]`` when the series layout hands statics
    or ids per item, ``[1, steps, N]`` when one block serves every item, else None), ``floor``, ``hist``, ``steps``.

    Filled in canonical batches: batch ``i`` is items ``i batch_size .. (i + 1) batch_size - 1`` in item order, the
    short last one included - ``windows.batch(i)`` of the default loader, ``windows.gather(arange)`` of a training
    loader - with one frozen forward (``model.output_inputs``) each.  The period selector averages amplitudes over a
    batch, so an item's ``seq`` depends on its batch: the cache defines it as that of the canonical batch (DESIGN.md
    section 8).  Windows that shift or add noise have no cache (ValueError).  ``bytes_needed`` is the size of the
    stores from the host alone; beyond ``max_bytes`` the constructor raises before it allocates.

    The cache remembers ``_param_key`` of every parameter outside the six refit tensors and each block's engine;
    ``check(model)`` raises ValueError when they differ.  A step of the six tensors does not invalidate it.

    ``late_bias=True`` (a refit that moves the late-bias head): in place of ``late`` the cache keeps what that head
    reads, the frozen series rows ``rows`` (``TimesNet.late_rows``) - ``[n_items, ctx]`` where ``late`` would be per
    item, the shared ``[1, N, ctx]`` block otherwise - and its key leaves out the head's five tensors as well.  A model
    without the head is a ValueError."""

    def __init__(self, model, windows, use_loss_mask: bool = False, max_bytes: Optional[int] = None,
                 late_bias: bool = False):
        from .score import _unpack_batch

        self._refuse_augmented(windows)
        self.late_bias = bool(late_bias)
        if self.late_bias:
            _late_params(model)
        need = self.bytes_needed(model, windows, use_loss_mask, late_bias=self.late_bias)
        if max_bytes is not None and need > int(max_bytes):
            raise ValueError(f"OutputCache: the stores need {need} bytes, max_bytes is {int(max_bytes)}")
        n, B = windows.n_items, windows.batch_size
        dev = _refit_params(model)[0].device
        self.windows, self.use_loss_mask = windows, bool(use_loss_mask)
        self.steps = int(model._out_steps)
        self.hist = min(self.steps, int(model.input_len))
        self.n_items, self.batch_size = n, B
        layout = _late_layout(model, windows)
        if self.late_bias and layout is None:
            raise ValueError("OutputCache: late_bias=True, but these windows give the late-bias head no series rows")
        self.seq = self.tail = self.y = self.mask = self.late = self.floor = self.rows = None
        was_training = model.training
        model.eval()
        try:
            for k0 in range(0, n, B):
                k1 = min(k0 + B, n)
                batch = windows.batch(k0 // B) if windows._default else \
                    windows.gather(torch.arange(k0, k1, dtype=torch.int64, device=windows.device))
                xb, yb, mask, x_mark, _, static, ids = _unpack_batch(batch)
                move = lambda t: None if t is None else t.to(dev, non_blocking=True)
                ids_d = None if ids is None else ids.to(device=dev, dtype=torch.long, non_blocking=True)
                seq, tail, hist, late, floor = model.output_inputs(move(xb), move(x_mark), move(static), ids_d)
                srows = model.late_rows(move(xb), move(x_mark), move(static), ids_d) if self.late_bias else None
                if use_loss_mask and mask is None:
                    raise ValueError("OutputCache: use_loss_mask needs a mask in every batch")
                got = None if late is None else ("shared" if layout != "item" and late.shape[0] == 1 else "item")
                if got != layout or hist != self.hist:
                    raise ValueError(f"OutputCache: the late bias came out as {got!r} where the model's layers said "
                                     f"{layout!r}; call the model on a batch of these windows before caching them")
                if self.seq is None:
                    N = tail.shape[2]
                    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
                    self.seq, self.tail = new(n, *seq.shape[1:]), new(n, hist, N)
                    self.y = new(n, self.steps, N)
                    self.mask = new(n, self.steps, N) if use_loss_mask else None
                    self.late = new(n if layout == "item" else 1, self.steps, N) if layout and not self.late_bias \
                        else None
                    if self.late_bias:
                        self.rows = new(n, srows.shape[2]) if layout == "item" else new(1, N, srows.shape[2])
                    self.floor = None if floor is None else floor.to(device=dev, dtype=torch.float32).clone()
                self.seq[k0:k1].copy_(seq)
                self.tail[k0:k1].copy_(tail)
                self.y[k0:k1].copy_(move(yb)[:, :self.steps, :])
                if use_loss_mask:
                    self.mask[k0:k1].copy_(move(mask)[:, :self.steps, :] > 0.0)
                if self.late_bias:
                    if layout == "item":                        # the series layout: N == 1, a row an item
                        self.rows[k0:k1].copy_(srows.expand(k1 - k0, -1, -1).reshape(k1 - k0, -1))
                    elif k0 == 0:
                        self.rows.copy_(srows)
                elif layout == "item":
                    self.late[k0:k1].copy_(late.expand(k1 - k0, -1, -1))
                elif layout == "shared" and k0 == 0:
                    self.late.copy_(late)
        finally:
            model.train(was_training)
        if self.seq is None:
            raise ValueError("OutputCache: the windows have no items")
        self.late_per_item = layout == "item"
        self.min_sigma = float(model.min_sigma)
        self.late_eps = float(model.late_bias_norm.eps) if self.late_bias else None
        self._key = self._backbone_key(model, self.late_bias)

    @staticmethod
    def _refuse_augmented(windows) -> None:
        if windows.time_shift or windows.add_noise_std:
            raise ValueError(f"OutputCache: windows with time_shift={windows.time_shift} / add_noise_std="
                             f"{windows.add_noise_std} differ per epoch and have no cache")

    @staticmethod
    def bytes_needed(model, windows, use_loss_mask: bool = False, late_bias: bool = False) -> int:
        """The bytes of ``seq``, ``tail``, ``y``, ``mask`` and ``late`` (with ``late_bias``: the series rows in its
        place) for these windows, from the host alone (the model's lazily built layers must exist: call it once
        first)."""
        if model.d_model is None:
            raise ValueError("OutputCache.bytes_needed: the model has not been called yet (d_model is unknown)")
        n, L, D = windows.n_items, int(model.input_len), int(model.d_model)
        N = 1 if windows.layout == "series" else windows.n_series
        steps = int(model._out_steps)
        layout = _late_layout(model, windows)
        late = {None: 0, "shared": 1, "item": n}[layout]
        late_floats = late * steps * N
        if late_bias and layout is not None:
            late_floats = late * N * int(model.late_bias_head.in_features)
        return 4 * (n * L * D + n * min(steps, L) * N + (2 if use_loss_mask else 1) * n * steps * N + late_floats)

    @property
    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size()
                   for t in (self.seq, self.tail, self.y, self.mask, self.late, getattr(self, "rows", None))
                   if t is not None)

    @staticmethod
    def _backbone_key(model, late_bias: bool = False):
        from .models.timesnet import _param_key

        six = {id(p) for p in _refit_params(model) + (_late_params(model) if late_bias else [])}
        return (_param_key([p for p in model.parameters() if id(p) not in six]),
                tuple(getattr(b, "engine", None) for b in model.blocks))

    def check(self, model) -> None:
        if self._backbone_key(model, getattr(self, "late_bias", False)) != self._key:
            raise ValueError("OutputCache: the backbone changed since the cache was filled")

    def select(self, rows: torch.Tensor):
        """``(tail, y, mask, late)`` of the batch ``rows`` by ``index_select`` (the eager step's operands): the mask
        as bool, the late bias as its shared block where it has one."""
        pick = lambda t: None if t is None else t.index_select(0, rows)
        return (pick(self.tail), pick(self.y), None if self.mask is None else pick(self.mask) > 0.0,
                pick(self.late) if self.late_per_item else self.late)

    def late_of(self, model, rows: torch.Tensor) -> torch.Tensor:
        """The late bias of the batch ``rows`` from the cached series rows and the model's late-bias head as it is now
        (``late_bias`` caches): ``late_bias``' node, so a backward reaches the head's five tensors."""
        return _late_bias_node(self.rows, *_late_params(model), self.late_eps,
                               index=rows if self.late_per_item else None)


class GraphedCachedStep:
    """``GraphedRefitStep`` without the backbone: a step of the output side on the items ``rows`` of an
    ``OutputCache``, captured once and replayed with one graph launch.  The captured launches are
    ``ftn_refit_rows_gather`` (tail, y, mask and a per-item late bias into batch tensors; the clamped list and the
    status word), ``ftn_timeproj_forward_rows`` on the cached ``seq`` in place, ``ftn_head_fit_forward``,
    ``ftn_nb_nll_grad``, ``ftn_head_backward``, ``ftn_timeproj_backward_rows`` into the last ``steps`` rows of zeroed
    full-size buffers, and ``optimizer.step_on`` with the heads' ``bad`` word and the status word as skip words.
    ``step(rows)`` copies an int64 device vector of ``batch_size`` items (a slice of ``windows.order(e)``) into the
    captured list ``.rows`` and replays.  An index outside the cache is clamped by every kernel and skips the update
    (flag 8 in the optimizer's log): neither a fault nor an unnoticed wrong step.  Nothing is read on the host.
    ``extra_skip``: further skip words of ``step_on`` behind those two (``EpochEnd.stop``); the default adds none.

    ``late_bias=True`` (a cache filled with ``late_bias=True``, a ``DeviceAdamWList`` over the eleven tensors): the
    step also captures ``ftn_late_fit_forward`` on the cached series rows (through the clamped row list where they
    are per item), ``d_pre = g_rate sig_mu scale`` as torch ops (summed over the batch where one block of rows serves
    it, as the eager node's incoming gradient is), ``ftn_late_backward``, and the update is
    ``ftn_refit_update_list`` over all eleven."""

    def __init__(self, cache: OutputCache, model, optimizer: DeviceAdamW, batch_size: int, warmup: int = 2,
                 extra_skip=(), late_bias: bool = False):
        if not isinstance(optimizer, DeviceAdamW):
            raise ValueError("GraphedCachedStep needs a fit.DeviceAdamW")
        self.extra_skip = list(extra_skip)
        self.late_bias = bool(late_bias)
        if self.late_bias != bool(getattr(cache, "late_bias", False)):
            raise ValueError("GraphedCachedStep: late_bias must be that of the cache")
        params = _refit_params(model) + (_late_params(model) if self.late_bias else [])
        if len(optimizer.params) != len(params) or any(a is not b for a, b in zip(optimizer.params, params)):
            raise ValueError("GraphedCachedStep: the optimizer must hold mu_head, sigma_head and forecast_time_proj "
                             "(weight, bias each, in that order)" +
                             (", then late_bias_norm, late_bias_head (weight, bias each) and late_bias_gate"
                              if self.late_bias else ""))
        dev = params[0].device
        D = cache.seq.shape[2]
        if (dev.type != "cuda" or cache.seq.device != dev
                or any(p.dtype != torch.float32 or not p.is_contiguous() for p in params)
                or not (D % 4 == 0 and 4 <= D <= 512 and cache.seq.data_ptr() % 16 == 0
                        and params[0].data_ptr() % 16 == 0 and params[2].data_ptr() % 16 == 0)):
            raise ValueError("GraphedCachedStep needs a cache and a model with contiguous fp32 parameters on one ROCm "
                             "device whose output side takes the HIP path (d_model a multiple of 4 up to 512, weights "
                             "on the 16-byte grid)")
        cache.check(model)
        B = int(batch_size)
        if B < 1:
            raise ValueError(f"GraphedCachedStep: batch_size={batch_size} is not positive")
        self.cache, self.model, self.optimizer, self.device, self.batch_size = cache, model, optimizer, dev, B
        self.steps = cache.steps
        N = cache.y.shape[2]
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        self._rows = torch.zeros(B, dtype=torch.int64, device=dev)
        self._rows_ok = torch.zeros(B, dtype=torch.int64, device=dev)
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        self._batch = (new(B, cache.hist, N), new(B, cache.steps, N),
                       None if cache.mask is None else new(B, cache.steps, N),
                       new(B, cache.steps, N) if cache.late_per_item and cache.late is not None else None)
        proj = model.forecast_time_proj
        self._gw, self._gb = torch.zeros_like(proj.weight), torch.zeros_like(proj.bias)   # rows before -steps stay 0
        # warm-up on a side stream, as GraphedRefitStep: the update goes to copies and a throw-away optimizer
        spare = type(optimizer)([p.detach().clone() for p in params], backend="hip")
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side), torch.no_grad():
            for _ in range(max(1, int(warmup))):
                self._enqueue(spare)
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        self.graph = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(self.graph):
            self.loss, self.bad, self.grads, self._keep = self._enqueue(optimizer)

    def _enqueue(self, optimizer: DeviceAdamW):
        """The step's launches on the current stream."""
        from . import runtime as rt

        cache, steps = self.cache, self.steps
        w_mu, b_mu, w_sg, b_sg, pw, pb = (p.detach() for p in _refit_params(self.model))
        late_ps = [p.detach() for p in _late_params(self.model)] if self.late_bias else None
        tail, y, mask, late, rows_ok, status = rt.refit_rows_gather(
            self._rows, cache.tail, cache.y, cache.mask, cache.late if cache.late_per_item else None,
            out=self._batch, rows_ok=self._rows_ok, status=self.status)
        if self.late_bias:
            late = rt.late_fit_forward(cache.rows, *late_ps, cache.late_eps,
                                       rows=rows_ok if cache.late_per_item else None)
        elif not cache.late_per_item:
            late = cache.late
        hidden = rt.timeproj_forward(cache.seq, pw[-steps:], pb[-steps:], rows=rows_ok)
        rate, disp, sig_mu, sig_sg, bad = rt.head_fit_forward(hidden, w_mu, b_mu.contiguous(), w_sg, b_sg.contiguous(),
                                                              tail, cache.hist, late, cache.floor, cache.min_sigma)
        words, g_rate, g_disp = rt.nb_nll_grad(y, rate, disp, mask, scaled=False)
        dw_mu, db_mu, dw_sg, db_sg, d_hidden = rt.head_backward(hidden, g_rate, g_disp, sig_mu, sig_sg,
                                                                words[1:2], w_mu, w_sg, want_hidden=True)
        rt.timeproj_backward(cache.seq, d_hidden, dw=self._gw[-steps:], db=self._gb[-steps:], rows=rows_ok)
        grads = [dw_mu, db_mu, dw_sg, db_sg, self._gw, self._gb]
        d_pre = None
        if self.late_bias:                                      # what _HeadNLL.backward hands the eager node
            d_pre = g_rate * sig_mu * words[1:2]
            if not cache.late_per_item and d_pre.shape[0] > 1:
                d_pre = d_pre.sum(0, keepdim=True)
            d_late = rt.late_backward(d_pre, cache.rows, *late_ps, cache.late_eps,
                                      rows=rows_ok if cache.late_per_item else None)
            grads = grads + list(d_late[:4]) + [d_late[4].view(late_ps[4].shape)]
        optimizer.step_on(grads, loss=words[0:1], skip=[bad, status] + self.extra_skip)
        keep = (hidden, rate, disp, sig_mu, sig_sg, words, g_rate, g_disp, d_hidden, late, d_pre)
        return words[0:1], bad, grads, keep

    @property
    def rows(self) -> torch.Tensor:
        """The captured row list (int64 ``[batch_size]``); writing into it saves ``step``'s copy."""
        return self._rows

    def replay(self) -> torch.Tensor:
        """One replay on the list as it is; returns the loss word (overwritten by the next replay)."""
        self.graph.replay()
        self.optimizer.note_replay()
        return self.loss

    def step(self, rows: torch.Tensor) -> torch.Tensor:
        if (not isinstance(rows, torch.Tensor) or rows.dtype != torch.int64 or tuple(rows.shape) != (self.batch_size,)
                or rows.device != self.device):
            raise ValueError(f"GraphedCachedStep.step: rows must be int64 [{self.batch_size}] on {self.device}")
        if rows.data_ptr() != self._rows.data_ptr():
            self._rows.copy_(rows, non_blocking=True)
        return self.replay()


def refit_output_cached(model, windows, epochs: int = 1, lr=1e-3, weight_decay: float = 0.0,
                        grad_clip: Optional[float] = None, use_loss_mask: bool = False,
                        cache: Optional[OutputCache] = None, graphed: bool = True, late_bias: bool = False):
    """``refit_output_graphed`` over an ``OutputCache``: the frozen backbone runs once per item (not at all with a
    ``cache`` given, which is ``check``ed and must be of these ``windows``), and every step of every epoch is the
    output side alone on ``windows.order(e)[i B : (i + 1) B]``, ``len(windows)`` batches an epoch.  A full batch is
    one replay of a ``GraphedCachedStep``; a short last batch, ``graphed=False`` and tensors the HIP path does not
    take run the eager step (``output_nll(..., rows=)`` and the same ``DeviceAdamW``).  ``lr``: a float, or one value
    per epoch.  ``windows.epoch`` advances as ``iter(windows)`` would advance it.  One synchronisation at the end,
    which raises what ``refit_output_graphed`` raises from the log, and IndexError when a step was skipped for a row
    outside the cache.  Returns the losses, fp32 ``[epochs * batches]`` on the host; mode and ``requires_grad`` flags
    come back as they were.  With ``shuffle=False`` the result has the bits of ``refit_output_graphed``; with
    ``shuffle=True`` the period selection is frozen with the backbone.

    ``late_bias=True``: the late-bias head moves with the six tensors - eleven in ``refit_output``'s order, one
    ``DeviceAdamWList`` step with ``grad_clip`` as the global norm over all of them; the cache keeps the frozen series
    rows in place of the late bias (a given ``cache`` must have been filled with ``late_bias=True``), and the series
    rows are frozen with the backbone.  A model without the head is a ValueError."""
    epochs = int(epochs)
    rates = [float(lr)] * epochs if isinstance(lr, (int, float)) else [float(v) for v in lr]
    if len(rates) != epochs:
        raise ValueError(f"refit_output_cached: {len(rates)} learning rates for {epochs} epochs")
    late_bias = bool(late_bias)
    if late_bias:
        _late_params(model)
    if cache is None:
        cache = OutputCache(model, windows, use_loss_mask=use_loss_mask, late_bias=late_bias)
    else:
        if cache.windows is not windows:
            raise ValueError("refit_output_cached: the cache was filled from other windows")
        if bool(getattr(cache, "late_bias", False)) != late_bias:
            raise ValueError("refit_output_cached: late_bias must be that of the cache")
        if use_loss_mask and cache.mask is None:
            raise ValueError("refit_output_cached: use_loss_mask needs a cache filled with use_loss_mask")
        OutputCache._refuse_augmented(windows)
        cache.check(model)
    params = _refit_params(model) + (_late_params(model) if late_bias else [])
    dev = params[0].device
    flags = [(p, p.requires_grad) for p in model.parameters()]
    was_training = model.training
    losses = []
    B, steps = windows.batch_size, cache.steps
    use_mask = use_loss_mask and cache.mask is not None
    try:
        for p, _ in flags:
            p.requires_grad_(False)
        for p in params:
            p.requires_grad_(True)
        model.eval()
        opt = (DeviceAdamWList if late_bias else DeviceAdamW)(params, lr=rates[0] if rates else 1e-3,
                                                              weight_decay=weight_decay, max_norm=grad_clip)
        step = None
        proj = model.forecast_time_proj
        for e in range(epochs):
            opt.set_lr(rates[e])
            epoch = windows.epoch
            if not windows._default:
                windows.epoch += 1
            order = windows.order(epoch).to(dev)
            for i in range(len(windows)):
                rows = order[i * B:(i + 1) * B]
                if graphed and dev.type == "cuda" and rows.numel() == B:
                    if step is None:
                        if not use_mask and cache.mask is not None:     # a cache with a mask, a refit without one
                            cache = _without_mask(cache)
                        step = GraphedCachedStep(cache, model, opt, B, late_bias=late_bias)
                    losses.append(step.step(rows).clone())
                    continue
                tail, y, mask, late = cache.select(rows)
                opt.zero_grad(set_to_none=True)
                with torch.enable_grad():
                    if late_bias:
                        late = cache.late_of(model, rows)
                    loss, bad = output_nll(cache.seq, proj.weight[-steps:], proj.bias[-steps:], *params[:4], tail,
                                           cache.hist, y, mask if use_mask else None, late, cache.floor,
                                           cache.min_sigma, rows=rows)
                loss.backward()
                opt.step(loss=loss.detach(), skip=[bad])
                opt.zero_grad(set_to_none=True)
                losses.append(loss.detach().reshape(1))
    finally:
        for p, flag in flags:
            p.requires_grad_(flag)
        model.train(was_training)
    if not losses:
        raise ValueError("refit_output_cached: no batches")
    host = torch.cat(losses).cpu()                               # the one synchronisation
    log = opt.history()
    seen = 0
    for v in log[:, 3].tolist():
        seen |= int(v)
    for bit, name in ((1, "rate"), (2, "dispersion")):
        if seen & bit:
            raise RuntimeError(f"Predicted {name} must be finite and strictly positive")
    if seen & 4:
        raise FloatingPointError("refit_output_cached: " + _RANGE_MESSAGE)
    # flag 8 beside a finite loss and norm is the status word of ftn_refit_rows_gather
    if bool(((log[:, 3].to(torch.int32) & 8) != 0).logical_and(torch.isfinite(log[:, :2]).all(1)).any()):
        raise IndexError("refit_output_cached: a step's row list pointed outside the cache; those steps were skipped")
    return host


def _without_mask(cache: OutputCache) -> OutputCache:
    """A view of ``cache`` whose steps use no mask (the stores are shared)."""
    import copy

    bare = copy.copy(cache)
    bare.mask = None
    return bare


# ------------------------------------------------------------------ validated refit: held-out NLL, best state, early stop
EPOCH_STOP, EPOCH_AFTER_STOP, EPOCH_SCORER_ERR = 16, 16, 32
_STATE_BYTES = 64                            # FtnEpochState: four fp64, then eight int32
_I_EPOCH, _I_BEST, _I_PATIENCE, _I_NUM_BAD, _I_STOP, _I_IMPROVED, _I_CALLS = range(8, 15)   # int32 words of the record
_last_epoch_backend: Optional[str] = None    # which path the last ``EpochEnd.end_epoch`` took


class ValidationAccumulators(ForecastScorer):
    """A ``ForecastScorer`` without ids whose every buffer is updated in place, so that ``update`` can sit in a
    captured graph and ``ftn_refit_epoch_end`` can read and clear the buffers on the device.  ``result()`` is the
    parent's and has the bits of a ``ForecastScorer(n_slots)`` fed the same batches, the "batch without a valid
    element" rule of ``_den_extra`` included.  ``reset`` zeroes in place."""

    def reset(self) -> None:
        if getattr(self, "_acc", None) is None:
            super().reset()
            return
        for t in (self._acc, self._err, self._den_extra, self._count_seen):
            t.zero_()

    def update(self, y, rate, dispersion, mask=None) -> None:                   # noqa: D102
        if y.dim() != 3 or rate.shape != y.shape or dispersion.shape != y.shape:
            raise ValueError(f"ValidationAccumulators.update takes y, rate, dispersion of one shape [B, H, N], got "
                             f"{tuple(y.shape)} {tuple(rate.shape)} {tuple(dispersion.shape)}")
        if y.shape[2] > self.n_slots:
            raise ValueError(f"{y.shape[2]} series need {y.shape[2]} slots, the accumulators have {self.n_slots}")
        if self.device.type == "cuda":
            self._update_hip(y, rate, dispersion, mask, None)
        else:
            self._update_torch(y, rate, dispersion, mask, None)
        _, counts = _part_views(self._acc)
        seen = counts[:, 0].sum(dtype=torch.int64)
        self._den_extra += (seen == self._count_seen).to(torch.float64) * float(y.numel())
        self._count_seen.copy_(seen)


def _epoch_rule(who: str, patience, plateau):
    """``(patience limit or None, (factor, patience, threshold, min_lr) or None)`` after the host's checks.
    ``plateau``: a dict with torch's ``ReduceLROnPlateau`` names and defaults (``factor`` 0.1, ``patience`` 10,
    ``threshold`` 1e-4, ``min_lr`` 0), or those four values as a tuple."""
    if patience is not None:
        if isinstance(patience, bool) or not isinstance(patience, int) or patience < 0:
            raise ValueError(f"{who}: patience={patience!r} is not None or an int >= 0")
    if plateau is None:
        return patience, None
    if isinstance(plateau, dict):
        odd = set(plateau) - {"factor", "patience", "threshold", "min_lr"}
        if odd:
            raise ValueError(f"{who}: plateau has unknown keys {sorted(odd)}")
        plateau = (plateau.get("factor", 0.1), plateau.get("patience", 10), plateau.get("threshold", 1e-4),
                   plateau.get("min_lr", 0.0))
    if not isinstance(plateau, (tuple, list)) or len(plateau) != 4:
        raise ValueError(f"{who}: plateau is a dict or (factor, patience, threshold, min_lr)")
    factor, p_pat, threshold, min_lr = plateau
    if isinstance(p_pat, bool) or not isinstance(p_pat, int) or p_pat < 0:
        raise ValueError(f"{who}: plateau patience={p_pat!r} is not an int >= 0")
    factor, threshold, min_lr = float(factor), float(threshold), float(min_lr)
    if not (0.0 < factor < 1.0 and threshold == threshold and min_lr >= 0.0):
        raise ValueError(f"{who}: plateau factor={factor} (inside (0, 1)), threshold={threshold}, min_lr={min_lr} (>= 0)")
    return patience, (factor, p_pat, threshold, min_lr)


class EpochEnd:
    """The end of a validated refit's epoch with nothing read on the host (the reference's train.py:1536-1572): from
    the validation sums in ``accumulators`` it computes ``val_nll`` and ``val_smape`` as ``ForecastScorer.result()``
    does, steps ``ReduceLROnPlateau`` (mode ``min``, relative threshold, no cooldown, eps 1e-8) on ``val_nll`` and
    writes the optimizer's ``lr`` word, keeps the parameters of the best epoch (``val_nll < best_nll``, strict; a NaN
    is never better) in ``best``, counts epochs without improvement and sets the word ``stop`` to 16 beyond
    ``patience`` of them - which, as a bare skip word of ``DeviceAdamW``, makes every later step keep all its bits -
    logs a row, and clears the accumulators.  A call after the stop only logs a row (flag 16) and clears.

    ``ftn_refit_epoch_end`` (``csrc/refit_epoch.hip``: one deciding workgroup, then a copy grid) on contiguous fp32
    ROCm parameters (backend ``hip``), the same rule in torch ops with ``torch.where`` anywhere else (backend
    ``torch``; on the CPU its sums are serial and have the kernel's bits); ``_last_epoch_backend`` says which ran.
    ``state`` is the ``FtnEpochState`` record, ``stop`` / ``improved`` one-element int32 views of it, ``log`` fp64
    ``[max_epochs, 5]`` rows ``(val_nll, val_smape, lr after, flags, improved)`` - without ``plateau`` the ``lr``
    column is the optimizer's word as the epoch left it.  Flags: 16 after the stop, 32 the scorer's error word."""

    def __init__(self, params, n_slots: int, max_epochs: int, lr: float, patience: Optional[int] = None,
                 plateau=None, backend: Optional[str] = None):
        self.params = list(params)
        if not 1 <= len(self.params) <= 8:
            raise ValueError(f"EpochEnd: {len(self.params)} parameter tensors (1..8)")
        for p in self.params:
            if not isinstance(p, torch.Tensor) or not p.is_floating_point() or p.numel() < 1:
                raise ValueError("EpochEnd: parameters must be floating-point tensors that are not empty")
        if len({p.device for p in self.params}) != 1:
            raise ValueError("EpochEnd: parameters must be on one device")
        if int(n_slots) < 1 or int(max_epochs) < 1:
            raise ValueError(f"EpochEnd: n_slots={n_slots} and max_epochs={max_epochs} must be >= 1")
        if not float(lr) >= 0.0:
            raise ValueError(f"EpochEnd: lr={lr} must be >= 0")
        if backend not in (None, "hip", "torch"):
            raise ValueError(f"EpochEnd: backend {backend!r} is not 'hip', 'torch' or None")
        self.patience, self.plateau = _epoch_rule("EpochEnd", patience, plateau)
        self.backend, self.max_epochs = backend, int(max_epochs)
        dev = self.device = self.params[0].device
        self.state = torch.zeros(_STATE_BYTES, dtype=torch.uint8, device=dev)
        self._f64, self._i32 = self.state.view(torch.float64), self.state.view(torch.int32)
        self._f64[:3] = float("inf")
        self._f64[3] = float(lr)
        self.stop, self.improved = self._i32[_I_STOP:_I_STOP + 1], self._i32[_I_IMPROVED:_I_IMPROVED + 1]
        self.log = torch.zeros(self.max_epochs, 5, dtype=torch.float64, device=dev)
        self.best = [p.detach().clone(memory_format=torch.contiguous_format) for p in self.params]
        self.accumulators = ValidationAccumulators(int(n_slots), dev)

    def _hip(self) -> bool:
        eligible = self.device.type == "cuda" and all(p.dtype == torch.float32 and p.is_contiguous()
                                                      for p in self.params)
        return _use_hip("EpochEnd", self.backend, eligible, "contiguous fp32 parameters on a ROCm device")

    def end_epoch(self, optimizer) -> None:
        """The epoch's decision from the accumulators as they are; ``optimizer``: the ``DeviceAdamW`` whose ``lr``
        word a plateau schedule writes.  Enqueues only, and can be captured."""
        global _last_epoch_backend
        lr_word = getattr(optimizer, "_lr", None)
        if (not isinstance(lr_word, torch.Tensor) or lr_word.dtype != torch.float32 or lr_word.numel() != 1
                or lr_word.device != self.device):
            raise ValueError("EpochEnd.end_epoch needs the DeviceAdamW of these parameters (its lr word)")
        acc = self.accumulators
        if self._hip():
            from . import runtime as rt

            rt.refit_epoch_end(acc._acc, acc._err, acc._den_extra, acc._count_seen, self.state, lr_word, self.log,
                               self.patience, self.plateau, [p.detach() for p in self.params], self.best)
            _last_epoch_backend = "hip"
        else:
            with torch.no_grad():
                self._end_torch(lr_word)
            _last_epoch_backend = "torch"

    def _end_torch(self, lr_word: torch.Tensor) -> None:
        """``ftn_refit_epoch_end`` in torch ops: fp64 throughout, every decision a device word and every write a
        ``torch.where``.  ``cumsum`` from a leading 0.0 is the serial slot-order sum on the CPU."""
        acc, dev, f, i = self.accumulators, self.device, self._f64, self._i32
        f64 = dict(dtype=torch.float64, device=dev)
        sums, counts = _part_views(acc._acc)
        lead = torch.zeros(1, **f64)
        num = torch.cumsum(torch.cat([lead, sums[:, 0]]), 0)[-1]
        sm = torch.cumsum(torch.cat([lead, sums[:, 1]]), 0)[-1]
        cnt = counts.sum(0, dtype=torch.int64)
        den = cnt[0].double() + acc._den_extra.reshape(())
        nought = torch.zeros((), **f64)
        nll = torch.where(den > 0, num / den, nought)
        smape = torch.where(cnt[1] > 0, sm / cnt[1].double(), nought)
        for t in (acc._acc, acc._den_extra, acc._count_seen):
            t.zero_()
        best_nll, best_smape, p_best, lr_s = (f[k].clone() for k in range(4))
        epoch, best_epoch, pat, n_bad, stop, improved, calls = (i[k].clone() for k in range(_I_EPOCH, _I_CALLS + 1))
        live = stop == 0
        lr_now = lr_s if self.plateau is not None else lr_word.reshape(()).double()
        flags = (acc._err.reshape(()) != 0).to(torch.float64) * float(EPOCH_SCORER_ERR)
        epoch1 = epoch + 1
        lr1, p_best1, n_bad1 = lr_now, p_best, n_bad
        if self.plateau is not None:
            factor, p_pat, threshold, min_lr = self.plateau
            better = nll < p_best * (1.0 - threshold)
            p_best1 = torch.where(better, nll, p_best)
            n_bad1 = torch.where(better, torch.zeros_like(n_bad), n_bad + 1)
            cut = n_bad1 > p_pat
            new = torch.clamp(lr_now * factor, min=min_lr)
            lr1 = torch.where(cut & (lr_now - new > 1e-8), new, lr_now)
            n_bad1 = torch.where(cut, torch.zeros_like(n_bad1), n_bad1)
        up = nll < best_nll
        pat1 = torch.where(up, torch.zeros_like(pat), pat + 1)
        stop1 = torch.zeros_like(stop)
        if self.patience is not None:
            stop1 = torch.where(~up & (pat1 > self.patience), torch.full_like(stop, EPOCH_STOP), stop1)
        nan = torch.full((), float("nan"), **f64)
        row = torch.where(live, torch.stack([nll, smape, lr1, flags, up.to(torch.float64)]),
                          torch.stack([nan, nan, lr_now, nought + float(EPOCH_AFTER_STOP), nought]))
        at = torch.clamp(calls, max=self.max_epochs - 1).long().reshape(1)
        self.log.index_copy_(0, at, torch.where(calls < self.max_epochs, row.reshape(1, 5), self.log.index_select(0, at)))
        took = live & up
        f[0] = torch.where(took, nll, best_nll)
        f[1] = torch.where(took, smape, best_smape)
        f[2] = torch.where(live, p_best1, p_best)
        f[3] = torch.where(live, lr1, lr_s)
        i[_I_EPOCH] = torch.where(live, epoch1, epoch)
        i[_I_BEST] = torch.where(took, epoch1, best_epoch)
        i[_I_PATIENCE] = torch.where(live, pat1, pat)
        i[_I_NUM_BAD] = torch.where(live, n_bad1, n_bad)
        i[_I_STOP] = torch.where(live, stop1, stop)
        i[_I_IMPROVED] = torch.where(live, up.to(torch.int32), improved)
        i[_I_CALLS] = calls + 1
        if self.plateau is not None:
            lr_word.copy_(torch.where(live, lr1.to(torch.float32), lr_word.reshape(())).reshape(lr_word.shape))
        for p, b in zip(self.params, self.best):
            b.copy_(torch.where(took, p.detach(), b))

    def restore(self) -> None:
        """The best epoch's tensors back into the parameters; if no epoch improved they keep every bit.  Enqueues
        only."""
        if self._hip():
            from . import runtime as rt
            from .range_guard import _capturing

            rt.refit_epoch_restore(self.state, self.best, [p.detach() for p in self.params])
            if not _capturing():
                _bump_versions(self.params)
        else:
            with torch.no_grad():
                for p, b in zip(self.params, self.best):
                    p.copy_(torch.where(self._i32[_I_BEST] > 0, b, p.detach()))

    def history(self) -> dict:
        """``rows`` (the log rows of the calls so far, fp64 ``[calls, 5]`` on the host), ``epoch`` (epochs decided),
        ``best_epoch`` (1-based, 0: none improved), ``best_nll``, ``best_smape`` and ``stopped_epoch`` (the epoch that
        set the stop word, None if none did): one synchronisation."""
        host = torch.cat([self.log.reshape(-1), self._f64]).cpu()
        state = host[-_STATE_BYTES // 8:].clone()
        f, i = state.tolist(), state.view(torch.int32).tolist()
        calls = min(i[_I_CALLS], self.max_epochs)
        return {"rows": host[:-_STATE_BYTES // 8].reshape(-1, 5)[:calls].clone(), "epoch": i[_I_EPOCH],
                "best_epoch": i[_I_BEST], "best_nll": f[0], "best_smape": f[1],
                "stopped_epoch": i[_I_EPOCH] if i[_I_STOP] != 0 else None}


def _cached_forecast(cache: OutputCache, model, rows: torch.Tensor, out=None, rows_ok=None, status=None):
    """``(y, mask, rate, dispersion, bad, status)`` of the items ``rows`` of ``cache`` under the model's output side as
    it stands: on the device ``ftn_refit_rows_gather``, ``ftn_timeproj_forward_rows`` on the cached ``seq`` and the
    inference head kernel - the launches, and so the bits, of the model's own forward on that batch; elsewhere the
    torch composition.  ``status`` is the gather's word (4: an index was outside the cache and was clamped)."""
    steps = cache.steps
    w_mu, b_mu, w_sg, b_sg, pw, pb = (p.detach() for p in _refit_params(model))
    if cache.seq.is_cuda:
        from . import runtime as rt

        tail, y, mask, late, rows_ok, status = rt.refit_rows_gather(
            rows, cache.tail, cache.y, cache.mask, cache.late if cache.late_per_item else None,
            out=out, rows_ok=rows_ok, status=status)
        if not cache.late_per_item:
            late = cache.late
        hidden = rt.timeproj_forward(cache.seq, pw[-steps:], pb[-steps:], rows=rows_ok)
        rate, disp, bad = rt.head_forward(hidden, w_mu, b_mu.contiguous(), w_sg, b_sg.contiguous(), tail, cache.hist,
                                          late, cache.floor, cache.min_sigma)
        return y, mask, rate, disp, bad, status
    tail, y, mask, late = cache.select(rows)
    with torch.no_grad():
        hidden = torch.matmul(pw[-steps:], cache.seq.index_select(0, rows)) + pb[-steps:].view(1, -1, 1)
        rate, disp, bad = _heads_torch(hidden, w_mu, b_mu, w_sg, b_sg, tail, cache.hist, late, cache.floor,
                                       cache.min_sigma)
    return y, mask, rate, disp, bad, torch.zeros(1, dtype=torch.int32, device=rows.device)


class GraphedCachedEval:
    """One validation batch from an ``OutputCache``, captured once: ``ftn_refit_rows_gather``,
    ``ftn_timeproj_forward_rows`` on the cached ``seq``, the inference head kernel, then ``score_columns`` and
    ``score_fold`` into ``accumulators`` (``ValidationAccumulators.update``).  ``run(rows)`` copies an int64 device
    vector into the captured list and replays when it has ``batch_size`` entries; a shorter one takes the same
    launches eagerly.  The heads' ``bad`` word and the gather's status word are OR-ed into the sticky words
    ``bad_seen`` / ``rows_seen``: an index outside the cache is clamped and reported there.  Nothing is read on the
    host."""

    def __init__(self, cache: OutputCache, model, accumulators: ValidationAccumulators, batch_size: int,
                 warmup: int = 2):
        if not isinstance(accumulators, ValidationAccumulators):
            raise ValueError("GraphedCachedEval needs fit.ValidationAccumulators (EpochEnd.accumulators)")
        params = _refit_params(model)
        dev = params[0].device
        D = cache.seq.shape[2]
        if (dev.type != "cuda" or cache.seq.device != dev or accumulators.device != dev
                or any(p.dtype != torch.float32 or not p.is_contiguous() for p in params)
                or not (D % 4 == 0 and 4 <= D <= 512 and cache.seq.data_ptr() % 16 == 0
                        and params[0].data_ptr() % 16 == 0 and params[2].data_ptr() % 16 == 0)):
            raise ValueError("GraphedCachedEval needs a cache, accumulators and a model with contiguous fp32 "
                             "parameters on one ROCm device whose output side takes the HIP path (d_model a multiple "
                             "of 4 up to 512, weights on the 16-byte grid)")
        cache.check(model)
        B, N = int(batch_size), cache.y.shape[2]
        if B < 1:
            raise ValueError(f"GraphedCachedEval: batch_size={batch_size} is not positive")
        if N > accumulators.n_slots:
            raise ValueError(f"GraphedCachedEval: {N} series need {N} slots, the accumulators have "
                             f"{accumulators.n_slots}")
        self.cache, self.model, self.accumulators, self.device, self.batch_size = cache, model, accumulators, dev, B
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        self._rows = torch.zeros(B, dtype=torch.int64, device=dev)
        self._rows_ok = torch.zeros(B, dtype=torch.int64, device=dev)
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        self.bad_seen = torch.zeros(1, dtype=torch.int32, device=dev)
        self.rows_seen = torch.zeros(1, dtype=torch.int32, device=dev)
        self._batch = (new(B, cache.hist, N), new(B, cache.steps, N),
                       None if cache.mask is None else new(B, cache.steps, N),
                       new(B, cache.steps, N) if cache.late_per_item else None)
        # warm-up on a side stream into accumulators and sticky words of its own: the real ones do not move
        spare = ValidationAccumulators(accumulators.n_slots, dev)
        spare_words = (torch.zeros_like(self.bad_seen), torch.zeros_like(self.rows_seen))
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side), torch.no_grad():
            for _ in range(max(1, int(warmup))):
                self._enqueue(self._rows, spare, *spare_words, captured=True)
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        self.graph = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(self.graph):
            self._keep = self._enqueue(self._rows, accumulators, self.bad_seen, self.rows_seen, captured=True)

    def _enqueue(self, rows, accumulators, bad_seen, rows_seen, captured: bool):
        """The batch's launches on the current stream, into the captured buffers or (a short batch) fresh ones."""
        own = dict(out=self._batch, rows_ok=self._rows_ok, status=self.status) if captured else {}
        y, mask, rate, disp, bad, status = _cached_forecast(self.cache, self.model, rows, **own)
        accumulators.update(y, rate, disp, mask)
        bad_seen |= bad
        rows_seen |= status
        return y, mask, rate, disp, bad

    def run(self, rows: torch.Tensor) -> None:
        if (not isinstance(rows, torch.Tensor) or rows.dtype != torch.int64 or rows.dim() != 1
                or not 1 <= rows.numel() <= self.batch_size or rows.device != self.device):
            raise ValueError(f"GraphedCachedEval.run: rows must be int64 [1..{self.batch_size}] on {self.device}")
        if rows.numel() < self.batch_size:
            with torch.no_grad():
                self._enqueue(rows.contiguous(), self.accumulators, self.bad_seen, self.rows_seen, captured=False)
            return
        if rows.data_ptr() != self._rows.data_ptr():
            self._rows.copy_(rows, non_blocking=True)
        self.graph.replay()


class ValidatedRefit:
    """What ``refit_output_validated`` returns: ``losses`` (fp32, the steps of the epochs that ran), ``val_nll``,
    ``val_smape`` and ``lr`` (fp64, one value per epoch that ran), ``best_epoch`` (1-based; 0: no epoch improved),
    ``best_nll``, ``best_smape``, ``stopped_epoch`` (None if the epochs ran out), ``epochs_enqueued`` and
    ``optimizer`` (the loop's ``DeviceAdamW``: moments and step count as the last applied step left them)."""

    def __init__(self, losses, rows, best_epoch, best_nll, best_smape, stopped_epoch, epochs_enqueued, optimizer):
        self.losses, self.optimizer = losses, optimizer
        self.val_nll, self.val_smape, self.lr = rows[:, 0].clone(), rows[:, 1].clone(), rows[:, 2].clone()
        self.best_epoch, self.best_nll, self.best_smape = best_epoch, best_nll, best_smape
        self.stopped_epoch, self.epochs_enqueued = stopped_epoch, epochs_enqueued


def refit_output_validated(model, windows, val_windows, epochs: int, lr=1e-3, weight_decay: float = 0.0,
                           grad_clip: Optional[float] = None, use_loss_mask: bool = False,
                           patience: Optional[int] = None, plateau=None, restore_best: bool = True,
                           cache: Optional[OutputCache] = None, val_cache: Optional[OutputCache] = None,
                           sync_every: Optional[int] = None) -> ValidatedRefit:
    """``refit_output_cached`` with the reference's per-epoch validation (train.py:1536-1572) decided on the device:
    after each epoch's steps the held-out windows ``val_windows`` (a default loader: no shuffle, no augmentation) are
    scored from an ``OutputCache`` of their own - the backbone is frozen for them too - and ``EpochEnd`` steps the
    plateau schedule, keeps the best epoch's six tensors and sets the stop word, which every step takes as a further
    skip word.  ``patience``: epochs without a better ``val_nll`` that are tolerated (None: no early stop);
    ``plateau``: ``_epoch_rule``'s schedule, with which ``lr`` must be a float and the host never sets the rate again.
    ``sync_every=None``: every epoch is enqueued and the one synchronisation is at the end - steps after the stop keep
    every bit of parameters, moments and step count; ``sync_every=k``: the host reads the stop word after every k
    epochs and breaks.  ``restore_best`` puts the best epoch's tensors back at the end; if no epoch improved the last
    state stays, as the reference saves it.  Validation covers the model's ``_out_steps`` from the cache: for a direct
    model the reference's ``_eval_metrics``, for a recursive one the one-step held-out likelihood (DESIGN.md section
    8).  Raises what ``refit_output_cached`` raises, RuntimeError / IndexError for a validation batch likewise, and
    the scorer's ValueError for flag 32."""
    who = "refit_output_validated"
    epochs = int(epochs)
    if epochs < 1:
        raise ValueError(f"{who}: epochs={epochs} must be >= 1")
    scalar_lr = isinstance(lr, (int, float))
    if plateau is not None and not scalar_lr:
        raise ValueError(f"{who}: a list of learning rates and a plateau schedule exclude each other")
    rates = [float(lr)] * epochs if scalar_lr else [float(v) for v in lr]
    if len(rates) != epochs:
        raise ValueError(f"{who}: {len(rates)} learning rates for {epochs} epochs")
    patience, plateau = _epoch_rule(who, patience, plateau)
    if sync_every is not None and (isinstance(sync_every, bool) or not isinstance(sync_every, int) or sync_every < 1):
        raise ValueError(f"{who}: sync_every={sync_every!r} is not None or an int >= 1")
    if not val_windows._default or val_windows.time_shift or val_windows.add_noise_std:
        raise ValueError(f"{who}: val_windows must be a default loader (no shuffle, no augmentation)")
    if val_windows is windows:
        raise ValueError(f"{who}: val_windows are the training windows")
    caches = []
    for name, c, w in (("cache", cache, windows), ("val_cache", val_cache, val_windows)):
        if c is None:
            c = OutputCache(model, w, use_loss_mask=use_loss_mask)
        else:
            if c.windows is not w:
                raise ValueError(f"{who}: {name} was filled from other windows")
            if use_loss_mask and c.mask is None:
                raise ValueError(f"{who}: use_loss_mask needs a {name} filled with use_loss_mask")
            OutputCache._refuse_augmented(w)
            c.check(model)
        if not use_loss_mask and c.mask is not None:
            c = _without_mask(c)
        caches.append(c)
    cache, val_cache = caches
    if val_cache.y.shape[1:] != cache.y.shape[1:] or val_cache.seq.shape[1:] != cache.seq.shape[1:]:
        raise ValueError(f"{who}: the validation windows do not have the training windows' shapes")
    params = _refit_params(model)
    dev = params[0].device
    flags = [(p, p.requires_grad) for p in model.parameters()]
    was_training = model.training
    losses = []
    B, steps, per_epoch = windows.batch_size, cache.steps, len(windows)
    VB, n_val = val_windows.batch_size, val_windows.n_items
    if per_epoch < 1 or n_val < 1:
        raise ValueError(f"{who}: no batches")
    on_device = dev.type == "cuda"
    enqueued = 0
    try:
        for p, _ in flags:
            p.requires_grad_(False)
        for p in params:
            p.requires_grad_(True)
        model.eval()
        opt = DeviceAdamW(params, lr=rates[0], weight_decay=weight_decay, max_norm=grad_clip,
                          log_steps=min(max(4096, epochs * per_epoch), 1 << 20))
        end = EpochEnd(params, val_cache.y.shape[2], epochs, rates[0], patience, plateau)
        bad_seen = torch.zeros(1, dtype=torch.int32, device=dev)
        rows_seen = torch.zeros(1, dtype=torch.int32, device=dev)
        val_rows = torch.arange(n_val, dtype=torch.int64, device=dev)
        step = evaluator = None
        proj = model.forecast_time_proj
        for e in range(epochs):
            if plateau is None:
                opt.set_lr(rates[e])
            epoch = windows.epoch
            if not windows._default:
                windows.epoch += 1
            order = windows.order(epoch).to(dev)
            for i in range(per_epoch):
                rows = order[i * B:(i + 1) * B]
                if on_device and rows.numel() == B:
                    if step is None:
                        step = GraphedCachedStep(cache, model, opt, B, extra_skip=[end.stop])
                    losses.append(step.step(rows).clone())
                    continue
                tail, y, mask, late = cache.select(rows)
                opt.zero_grad(set_to_none=True)
                with torch.enable_grad():
                    loss, bad = output_nll(cache.seq, proj.weight[-steps:], proj.bias[-steps:], *params[:4], tail,
                                           cache.hist, y, mask, late, cache.floor, cache.min_sigma, rows=rows)
                loss.backward()
                opt.step(loss=loss.detach(), skip=[bad, end.stop])
                opt.zero_grad(set_to_none=True)
                losses.append(loss.detach().reshape(1))
            for k0 in range(0, n_val, VB):
                rows = val_rows[k0:k0 + VB]
                if on_device:
                    if evaluator is None:
                        evaluator = GraphedCachedEval(val_cache, model, end.accumulators, VB)
                    evaluator.run(rows)
                    continue
                y, mask, rate, disp, bad, status = _cached_forecast(val_cache, model, rows)
                end.accumulators.update(y, rate, disp, mask)
                bad_seen |= bad
                rows_seen |= status
            end.end_epoch(opt)
            enqueued += 1
            if sync_every is not None and enqueued % sync_every == 0 and int(end.stop.item()) != 0:
                break
        if restore_best:
            end.restore()
        if evaluator is not None:
            bad_seen, rows_seen = evaluator.bad_seen, evaluator.rows_seen
    finally:
        for p, flag in flags:
            p.requires_grad_(flag)
        model.train(was_training)
    host = torch.cat(losses).cpu()                               # the synchronisation at the end
    seen_val = torch.cat([bad_seen, rows_seen]).tolist()
    hist, log = end.history(), opt.history()
    ran = hist["stopped_epoch"] if hist["stopped_epoch"] is not None else enqueued
    first = opt._calls - log.shape[0]                            # the call the first returned row belongs to
    inside = torch.tensor([(first + k) // per_epoch < ran for k in range(log.shape[0])], dtype=torch.bool)
    log = log[inside]                                            # a step after the stop is skipped by design
    seen = seen_val[0]
    for v in log[:, 3].tolist():
        seen |= int(v) & 7
    for bit, name in ((1, "rate"), (2, "dispersion")):
        if seen & bit:
            raise RuntimeError(f"Predicted {name} must be finite and strictly positive")
    if seen & 4:
        raise FloatingPointError(f"{who}: " + _RANGE_MESSAGE)
    if bool(((log[:, 3].to(torch.int32) & 8) != 0).logical_and(torch.isfinite(log[:, :2]).all(1)).any()):
        raise IndexError(f"{who}: a step's row list pointed outside the cache; those steps were skipped")
    if seen_val[1]:
        raise IndexError(f"{who}: a validation batch's row list pointed outside the validation cache; the rows were "
                         "clamped into it")
    rows = hist["rows"][:ran]
    if bool((rows[:, 3].to(torch.int32) & EPOCH_SCORER_ERR).any()):
        raise ValueError(f"{who}: ForecastScorer: a series id outside the slots was given to the validation scorer")
    return ValidatedRefit(host[:ran * per_epoch], rows, hist["best_epoch"], hist["best_nll"], hist["best_smape"],
                          hist["stopped_epoch"], enqueued, opt)
