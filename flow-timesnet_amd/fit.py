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

``backend`` follows ``score``'s rule (``_use_hip``): ``hip`` where it can run unless ``"torch"`` is asked for, and
asking for ``"hip"`` where it cannot is an error.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from .score import _full_mask, _nb_ll_torch, _rows, _use_hip, negative_binomial_mask

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
    def forward(ctx, seq, wt, bt):
        from . import runtime as rt

        seq = seq.detach().contiguous()
        ctx.save_for_backward(seq)
        return rt.timeproj_forward(seq, wt.detach(), bt.detach())

    @staticmethod
    @once_differentiable
    def backward(ctx, d_hidden):
        from . import runtime as rt

        (seq,) = ctx.saved_tensors
        d_hidden = d_hidden.contiguous()
        if d_hidden.dtype != torch.float32 or d_hidden.data_ptr() % 16:     # (ftn_head_backward's own is neither)
            d_hidden = d_hidden.float().clone()
        dw, db = rt.timeproj_backward(seq, d_hidden)
        return None, dw if ctx.needs_input_grad[1] else None, db if ctx.needs_input_grad[2] else None


def time_projection(seq: torch.Tensor, wt: torch.Tensor, bt: torch.Tensor) -> torch.Tensor:
    """``hidden[b] = wt @ seq[b] + bt[:, None]``, ``[B, S, D]`` from ``seq [B, L, D]`` (``TimesNet.output_inputs``),
    ``wt [S, L]`` and ``bt [S]``, differentiable in ``wt`` and ``bt``.  ``wt`` / ``bt`` may be the row slices
    ``weight[-steps:]`` / ``bias[-steps:]`` of a taller projection: autograd scatters the gradient into the full
    parameter and the other rows get exact zeros.  On fp32 ROCm tensors with d_model a multiple of 4 up to 512 and a
    ``seq`` that does not require grad it is ``ftn_timeproj_forward`` (the bits of inference) with
    ``ftn_timeproj_backward`` as its backward (``_last_timeproj_backend == "hip"``); otherwise - CPU tensors, other
    dtypes, other widths, a ``seq`` that requires grad (no ``d_seq`` is computed here) - the torch composition
    ``torch.matmul(wt, seq) + bt.view(1, -1, 1)``."""
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
        return _TimeProjection.apply(seq, wt, bt)
    _last_timeproj_backend = "torch"
    return torch.matmul(wt, seq) + bt.view(1, -1, 1)


def output_nll(seq: torch.Tensor, wt: torch.Tensor, bt: torch.Tensor, w_mu: torch.Tensor, b_mu: torch.Tensor,
               w_sigma: torch.Tensor, b_sigma: torch.Tensor, tail: torch.Tensor, hist: int, y: torch.Tensor,
               mask: torch.Tensor | None = None, late: torch.Tensor | None = None, floor: torch.Tensor | None = None,
               min_sigma: float = 1e-3):
    """The whole output side on ``seq [B, L, D]`` (``TimesNet.output_inputs``): ``time_projection`` then ``head_nll``,
    ``(loss, bad)``.  ``loss.backward()`` leaves gradients in ``wt``, ``bt`` and the four head tensors; on the device
    path every one of them comes from ``ftn_head_backward`` (which also writes ``d_hidden``) and
    ``ftn_timeproj_backward``."""
    hidden = time_projection(seq, wt, bt)
    return head_nll(hidden, w_mu, b_mu, w_sigma, b_sigma, tail, hist, y, mask, late, floor, min_sigma)


def refit_output(model, batches, epochs: int = 1, lr: float = 1e-3, use_loss_mask: bool = False, optimizer=None,
                 grad_clip: Optional[float] = None):
    """``refit_heads`` over the whole output side of a ``TimesNet``: ``forecast_time_proj`` (its last
    ``model._out_steps`` rows are what a step reads; the other rows of a recursive model get zero gradients),
    ``mu_head`` and ``sigma_head``, everything else frozen.  Per batch ``model.output_inputs`` -> ``output_nll`` ->
    ``backward()`` -> (with ``grad_clip``, the reference's ``clip_grad_norm_`` over the six tensors, train.py:1513-1515)
    -> a step of ``optimizer`` (default: Adam with ``lr`` over the six tensors).  Losses and ``bad`` words stay on
    the device until the one synchronisation at the end, which raises the reference's RuntimeError if a rate or
    dispersion was not finite and > 0.  Returns the losses, fp32 ``[epochs * batches]`` on the host; mode and
    ``requires_grad`` flags come back as they were."""
    from .score import _unpack_batch

    proj = model.forecast_time_proj
    params = [model.mu_head.weight, model.mu_head.bias, model.sigma_head.weight, model.sigma_head.bias,
              proj.weight, proj.bias]
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
                opt.zero_grad(set_to_none=True)
                with torch.enable_grad():
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
