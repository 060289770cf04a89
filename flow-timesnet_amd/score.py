"""Scoring a probabilistic forecast where its outputs lie: the negative-binomial likelihood and the sMAPE of the
reference's ``losses.py`` / ``train._eval_metrics`` / ``utils/metrics.py``.

``negative_binomial_mask`` / ``negative_binomial_nll`` keep the reference's names and signatures.  Backends follow the
blocks' rule: ``hip`` for fp32 tensors on a ROCm device with nothing for autograd to record (``k_score_cols``, fp64
per-column sums, never a synchronisation), ``torch`` otherwise - the reference's function line by line.
``_last_backend`` records which ran.  One deliberate difference on the ``hip`` side: an invalid
element is excluded, where the reference multiplies its log-likelihood by a 0 weight and so turns one masked-out NaN
into a NaN mean.

``ForecastScorer`` accumulates per-slot sums over many batches (``update`` only enqueues; ``result`` makes the one
synchronisation), ``eval_metrics`` is ``_eval_metrics`` as a loop over batch tuples around it.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np
import torch

_last_backend: Optional[str] = None


def negative_binomial_mask(y: torch.Tensor, rate: torch.Tensor, dispersion: torch.Tensor,
                           mask: torch.Tensor | None = None) -> torch.Tensor:
    """Boolean mask of the valid NB likelihood elements (losses.py:6-24)."""
    finite_mask = torch.isfinite(y) & torch.isfinite(rate) & torch.isfinite(dispersion)
    if mask is not None:
        mask_bool = mask.to(dtype=torch.bool)
        if mask_bool.ndim < finite_mask.ndim:
            mask_bool = mask_bool.reshape(*mask_bool.shape, *([1] * (finite_mask.ndim - mask_bool.ndim)))
        mask_bool = mask_bool.expand_as(finite_mask)
        finite_mask = finite_mask & mask_bool
    return finite_mask


def _nb_ll_torch(y, rate, dispersion, eps):
    """``(ll, y, mu, alpha)`` of losses.py:36-53, fp32."""
    dtype = torch.float32
    y = torch.clamp(y.to(dtype), min=0.0)
    rate = rate.to(dtype)
    dispersion = dispersion.to(dtype)
    alpha = torch.clamp(dispersion, min=eps)
    mu = torch.clamp(rate, min=eps)
    log1p_alpha_mu = torch.log1p(alpha * mu)
    log_alpha = torch.log(alpha)
    log_mu = torch.log(mu)
    inv_alpha = torch.reciprocal(alpha)
    ll = (
        torch.lgamma(y + inv_alpha)
        - torch.lgamma(inv_alpha)
        - torch.lgamma(y + 1.0)
        + inv_alpha * (-log1p_alpha_mu)
        + y * (log_alpha + log_mu - log1p_alpha_mu)
    )
    return ll, y, mu, alpha


def _nll_torch(y, rate, dispersion, mask, eps):
    ll, y, mu, alpha = _nb_ll_torch(y, rate, dispersion, eps)
    valid_mask = negative_binomial_mask(y, mu, alpha, mask)
    weight = valid_mask.to(torch.float32)
    denom = torch.clamp(weight.sum(), min=1.0)
    return -(ll * weight).sum() / denom


def _hip_eligible(*tensors) -> bool:
    if not all(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 3
               for t in tensors):
        return False
    if len({t.device for t in tensors}) != 1 or len({tuple(t.shape) for t in tensors}) != 1 or tensors[0].numel() == 0:
        return False
    return not (torch.is_grad_enabled() and any(t.requires_grad for t in tensors))


def _rows(t: torch.Tensor) -> torch.Tensor:
    """``t`` [B,H,N] as the kernel takes it: rows contiguous and N apart (a batch stride of its own is fine)."""
    B, H, N = t.shape
    ok = (N == 1 or t.stride(2) == 1) and (H == 1 or t.stride(1) == N) and (B == 1 or t.stride(0) >= H * N)
    return t if ok else t.contiguous()


def _full_mask(mask, like: torch.Tensor):
    """None, or a contiguous [B,H,N] bool / uint8 / fp32 mask on ``like``'s device: the given one when it already is
    that, else the reference's broadcast (losses.py:17-22) materialised as uint8."""
    if mask is None:
        return None
    if (tuple(mask.shape) == tuple(like.shape) and mask.device == like.device and mask.is_contiguous()
            and mask.dtype in (torch.bool, torch.uint8, torch.float32)):
        return mask
    m = mask.to(device=like.device).to(dtype=torch.bool)
    if m.ndim < like.ndim:
        m = m.reshape(*m.shape, *([1] * (like.ndim - m.ndim)))
    return m.expand_as(like).contiguous()


def _part_views(part: torch.Tensor):
    """``(sums [n, 2] fp64 view of nll_sum | smape_sum, counts [n, 2] int32 view)`` of FtnScorePart storage."""
    n = part.numel() // 24
    f = part.view(torch.float64).view(n, 3)
    i = part.view(torch.int32).view(n, 6)
    return f[:, :2], i[:, 4:6]


def negative_binomial_nll(y: torch.Tensor, rate: torch.Tensor, dispersion: torch.Tensor,
                          mask: torch.Tensor | None = None, eps: float = 1e-8) -> torch.Tensor:
    """Negative binomial negative log-likelihood averaged over the valid elements (losses.py:27-58): a 0-dim
    tensor."""
    global _last_backend
    if _hip_eligible(y, rate, dispersion):
        from . import runtime as rt

        part, _ = rt.score_columns(_rows(y), _rows(rate), _rows(dispersion), _full_mask(mask, y), eps)
        sums, counts = _part_views(part)
        total = _ordered_sum(sums[:, 0])
        denom = counts[:, 0].sum().clamp(min=1).to(torch.float64)
        _last_backend = "hip"
        return (total / denom).to(torch.float32)
    _last_backend = "torch"
    return _nll_torch(y, rate, dispersion, mask, eps)


def _ordered_sum(v: torch.Tensor) -> torch.Tensor:
    """fp64 sum of a device vector, reproducible: cumsum's scan order depends on the length alone."""
    return torch.cumsum(v, 0)[-1]


def _smape_terms_torch(y, rate, valid):
    """The fp32 sMAPE terms of ``_eval_metrics`` + ``smape_mean`` and which of them count."""
    w = valid.to(y.dtype)
    a, p = y * w, rate * w
    counts = a.abs() > 1e-8
    terms = 2.0 * (p - a).abs() / (a.abs() + p.abs())
    return torch.where(counts, terms, torch.zeros_like(terms)), counts


class ForecastScorer:
    """Per-slot accumulators of the NB likelihood and the sMAPE over any number of batches.

    ``update(y, rate, dispersion, mask=None, series_ids=None)`` enqueues ``k_score_cols`` and ``k_score_fold`` and
    returns nothing; ``series_ids`` is None (slot = n), int64 [N] of distinct ids shared by the batch, or [B, N] with
    any repeats (the pipeline layout).  ``result()`` synchronises once.  Every slot's sums are taken one column at a
    time in ascending (b, n) order, so ``update(X); update(Y)`` leaves the bits of ``update(cat([X, Y]))``.  On CPU
    tensors the same class runs on torch ops in the same order."""

    def __init__(self, n_slots: int, device) -> None:
        if int(n_slots) < 1:
            raise ValueError(f"ForecastScorer: n_slots={n_slots}")
        self.n_slots = int(n_slots)
        self.device = torch.device(device)
        self._last_backend: Optional[str] = None
        self.reset()

    def reset(self) -> None:
        dev = self.device
        self._acc = torch.zeros(self.n_slots * 24, dtype=torch.uint8, device=dev)
        self._err = torch.zeros(1, dtype=torch.int32, device=dev)
        self._den_extra = torch.zeros((), dtype=torch.float64, device=dev)
        self._count_seen = torch.zeros((), dtype=torch.int64, device=dev)
        self._checked_ids: Dict[tuple, bool] = {}

    # ------------------------------------------------------------------ update
    def update(self, y, rate, dispersion, mask=None, series_ids=None) -> None:
        if y.dim() != 3 or rate.shape != y.shape or dispersion.shape != y.shape:
            raise ValueError(f"ForecastScorer.update takes y, rate, dispersion of one shape [B, H, N], got "
                             f"{tuple(y.shape)} {tuple(rate.shape)} {tuple(dispersion.shape)}")
        B, H, N = y.shape
        ids = None
        if series_ids is not None:
            ids = series_ids.to(device=self.device, dtype=torch.int64)
            if ids.dim() == 2 and ids.shape[0] == 1 and B > 1:
                ids = ids[0]
            if tuple(ids.shape) not in ((N,), (B, N)):
                raise ValueError(f"series_ids must be [N] or [B, N] = {(B, N)}, got {tuple(ids.shape)}")
        elif N > self.n_slots:
            raise ValueError(f"{N} series need {N} slots, the scorer has {self.n_slots}")
        if self.device.type == "cuda":
            self._update_hip(y, rate, dispersion, mask, ids)
        else:
            self._update_torch(y, rate, dispersion, mask, ids)
        # _eval_metrics counts a batch without one valid element with its numel in the denominator (train.py:745-749)
        _, counts = _part_views(self._acc)
        seen = counts[:, 0].sum(dtype=torch.int64)
        self._den_extra += (seen == self._count_seen).to(torch.float64) * float(y.numel())
        self._count_seen = seen

    def _update_hip(self, y, rate, dispersion, mask, ids) -> None:
        from . import runtime as rt

        y, rate, dispersion = (t.to(device=self.device, dtype=torch.float32) for t in (y, rate, dispersion))
        B, H, N = y.shape
        part, _ = rt.score_columns(_rows(y), _rows(rate), _rows(dispersion), _full_mask(mask, y))
        if ids is None:
            rt.score_fold(part, B, N, self._acc, self._err)
        elif ids.dim() == 1:
            key = (ids.data_ptr(), ids._version, N)
            if key not in self._checked_ids:                    # once per ids tensor: repeats inside a row would race
                self._checked_ids = {key: True}
                hist = torch.zeros(self.n_slots, dtype=torch.int32, device=self.device)
                hist.scatter_add_(0, ids.clamp(0, self.n_slots - 1), torch.ones_like(ids, dtype=torch.int32))
                self._err |= ((hist > 1).any().to(torch.int32) * 2)
            rt.score_fold(part, B, N, self._acc, self._err, ids=ids.contiguous())
        else:
            sorted_ids, order = torch.sort(ids.reshape(-1), stable=True)
            slots = torch.arange(self.n_slots + 1, dtype=torch.int64, device=self.device)
            rt.score_fold(part, B, N, self._acc, self._err, order=order,
                          seg_start=torch.searchsorted(sorted_ids, slots))
        self._last_backend = "hip"

    def _update_torch(self, y, rate, dispersion, mask, ids) -> None:
        y, rate, dispersion = (t.to(device=self.device, dtype=torch.float32) for t in (y, rate, dispersion))
        B, H, N = y.shape
        ll, yc, mu, alpha = _nb_ll_torch(y, rate, dispersion, 1e-8)
        valid = negative_binomial_mask(yc, mu, alpha, None if mask is None else mask.to(self.device))
        terms, counts = _smape_terms_torch(y, rate, valid)
        counts = counts & torch.isfinite(y)
        neg = torch.where(valid, -ll, torch.zeros_like(ll)).double()
        terms = torch.where(counts, terms, torch.zeros_like(terms)).double()
        sums = torch.zeros(B, N, 2, dtype=torch.float64)
        for h in range(H):                                      # h ascending, as the kernel's order within a segment
            sums[..., 0] += neg[:, h]
            sums[..., 1] += terms[:, h]
        cnts = torch.stack([valid.sum(1), counts.sum(1)], -1).to(torch.int32)
        acc_s, acc_c = _part_views(self._acc)
        if ids is not None and (int(ids.min()) < 0 or int(ids.max()) >= self.n_slots):
            self._err |= 1
            return
        for b in range(B):                                      # ascending (b, n): index_add_ on the CPU walks n in order
            slot = torch.arange(N) if ids is None else (ids if ids.dim() == 1 else ids[b])
            acc_s.index_add_(0, slot, sums[b])
            acc_c.index_add_(0, slot, cnts[b])
        self._last_backend = "torch"

    # ------------------------------------------------------------------ results
    def result(self) -> Dict[str, object]:
        """``nll`` and ``smape`` as ``_eval_metrics`` defines them, and the per-slot arrays ``nll_sum``,
        ``nll_count``, ``smape_sum``, ``smape_count`` (numpy).  The one synchronisation of a scoring run."""
        sums, counts = _part_views(self._acc)
        host = torch.cat([sums.reshape(-1), counts.reshape(-1).double(), self._err.double(),
                          self._den_extra.reshape(1)]).cpu().numpy()
        S = self.n_slots
        err = int(host[4 * S])
        if err & 1:
            raise ValueError(f"ForecastScorer: a series id outside [0, {S}) was given to update()")
        if err & 2:
            raise ValueError("ForecastScorer: series_ids of shape [N] repeat an id; pass them as [B, N]")
        s, c = host[:2 * S].reshape(S, 2), host[2 * S:4 * S].reshape(S, 2).astype(np.int64)
        nll_sum, smape_sum, nll_cnt, smape_cnt = s[:, 0].copy(), s[:, 1].copy(), c[:, 0].copy(), c[:, 1].copy()
        den = float(nll_cnt.sum()) + float(host[4 * S + 1])
        num, sm = 0.0, 0.0
        for v in nll_sum:                                       # slot order: the scalars are reproducible too
            num += float(v)
        for v in smape_sum:
            sm += float(v)
        n_sm = int(smape_cnt.sum())
        return {"nll": num / den if den > 0 else 0.0, "smape": sm / n_sm if n_sm > 0 else 0.0,
                "nll_sum": nll_sum, "nll_count": nll_cnt, "smape_sum": smape_sum, "smape_count": smape_cnt}

    def wsmape_grouped(self, ids: List[str], weights: Optional[Dict[str, float]] = None) -> float:
        """The reference's ``wsmape_grouped`` (utils/metrics.py:7-51) from the per-slot sMAPE means: ``ids[j]`` is
        ``"store_menu"`` of slot j; a slot without a point that counts scores 0."""
        r = self.result()
        if len(ids) != self.n_slots:
            raise ValueError(f"wsmape_grouped takes one id per slot ({self.n_slots}), got {len(ids)}")
        item = np.where(r["smape_count"] > 0, r["smape_sum"] / np.maximum(r["smape_count"], 1), 0.0)
        store_to_idx: Dict[str, List[int]] = {}
        for j, s in enumerate(ids):
            store_to_idx.setdefault(s.split("_", 1)[0], []).append(j)
        if weights is None:
            weights = {st: 1.0 for st in store_to_idx}
        Z = sum(weights.values()) if weights else 1.0
        score = 0.0
        for st, idxs in store_to_idx.items():
            score += (weights.get(st, 0.0) / Z) * float(np.mean(item[idxs]))
        return float(score)


def _unpack_batch(batch):
    """The reference's ``_unpack_batch`` (train.py:357-390): ``(xb, yb, mask[, x_mark, y_mark][, static[, ids]])``."""
    if not isinstance(batch, (list, tuple)):
        raise TypeError("batch must be a tuple or list of tensors")
    if len(batch) < 3:
        raise ValueError(f"Unexpected batch size: {len(batch)}")
    xb, yb, mask = batch[0], batch[1], batch[2]
    nxt, x_mark, y_mark, static, series_ids = 3, None, None, None, None
    if len(batch) >= 5:
        x_mark, y_mark, nxt = batch[3], batch[4], 5
        x_mark = None if x_mark is None or x_mark.numel() == 0 else x_mark
        y_mark = None if y_mark is None or y_mark.numel() == 0 else y_mark
    if len(batch) > nxt:
        static, nxt = batch[nxt], nxt + 1
    if len(batch) > nxt:
        series_ids, nxt = batch[nxt], nxt + 1
    if len(batch) != nxt:
        raise ValueError(f"Unexpected batch size: {len(batch)}")
    return xb, yb, mask, x_mark, y_mark, static, series_ids


def eval_metrics(model, batches, mode: str, pred_len: int, use_loss_mask: bool = False,
                 n_series: Optional[int] = None, scorer: Optional[ForecastScorer] = None) -> Dict[str, object]:
    """``_eval_metrics`` (train.py:675-765) over an iterable of batch tuples, on the model's device: the forward (or
    ``forecast.forecast_recursive_batch`` for ``mode="recursive"``) feeds a ``ForecastScorer`` of ``n_series`` slots
    (default: N of the first batch) and nothing of the scoring synchronises before the result is read.  Returns the
    scorer's ``result()``."""
    from . import forecast as fc

    dev = next(model.parameters()).device
    model.eval()
    with torch.inference_mode():
        for batch in batches:
            xb, yb, mask, x_mark, y_mark, static, ids = _unpack_batch(batch)
            xb, yb = xb.to(dev, non_blocking=True), yb.to(dev, non_blocking=True)
            base = (mask.to(dev, non_blocking=True) > 0.0) if use_loss_mask else None
            x_mark = None if x_mark is None else x_mark.to(dev, non_blocking=True)
            y_mark = None if y_mark is None else y_mark.to(dev, non_blocking=True)
            static = None if static is None else static.to(dev, non_blocking=True)
            ids = None if ids is None else ids.to(device=dev, dtype=torch.long, non_blocking=True)
            if scorer is None:
                scorer = ForecastScorer(int(n_series) if n_series is not None else yb.shape[2], dev)
            if mode == "direct":
                rate, disp = fc._invoke_model(model, xb, x_mark, static, ids)
            else:
                rate, disp = fc.forecast_recursive_batch(model, xb, pred_len, x_mark=x_mark, y_mark=y_mark,
                                                         series_static=static, series_ids=ids)
                rate, disp = rate[:, :yb.shape[1], :], disp[:, :yb.shape[1], :]
            scorer.update(yb, rate, disp, base, ids)
    if scorer is None:
        raise ValueError("eval_metrics: no batches")
    return scorer.result()
