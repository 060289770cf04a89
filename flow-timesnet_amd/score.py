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

``nb_cdf`` / ``nb_quantiles`` / ``prediction_interval`` / ``interval_metrics`` use the distribution itself (no
counterpart in the reference): the regularised incomplete beta function and its inversion, ``k_nb_cdf`` /
``k_nb_quantile`` on the ``hip`` side and the same method in fp64 torch ops otherwise (``nbdist``).

``nb_sample`` / ``sample_uniforms`` / ``path_quantiles`` draw from it: a counter-based Philox4x32-10 and the inversion
of that CDF (``k_nb_sample``, or the same generator and search in torch ops, ``nbdist``), so a draw is a pure function
of ``(seed, offset, element, draw index)``; ``forecast.forecast_sample_paths`` feeds the draws back into the recursion.

``path_summary`` / ``path_metrics`` summarise sample paths [P,B,H,N]: order statistics, mean and sample CRPS of window
sums or maxima, ``ftn_path_summary`` on the ``hip`` side (one pass over the paths, one sort per column in registers or
LDS) and the same definitions in fp64 torch ops otherwise.

``SeriesGroups`` / ``group_sums`` / ``group_path_summary`` / ``group_path_metrics`` total series over groups (a store's
items, the whole site) before summarising: a segmented sum along the series axis in a stated order,
``ftn_group_sum`` on the ``hip`` side and the same additions in fp64 torch ops otherwise, bit for bit.  With ``axis``
the series may lie along any dim - the pipeline's one series per batch row, samples [P,B,H,1] with ``axis=1`` -
(``ftn_group_sum_rows``, no copy), to the same bits.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional

import numpy as np
import torch

from .lib import (FTN_GROUP_CHUNK as GROUP_CHUNK, FTN_GROUP_CHUNKS_MAX as GROUP_CHUNKS_MAX,  # importing it loads nothing
                  FTN_GROUP_GMAX as GROUP_GMAX, FTN_GROUP_NMAX as GROUP_NMAX)
from .nbdist import (NBQ_FLAG_RANGE, NBQ_KLIM, NBQ_QMAX, _M32, _nb_cdf_torch, _nb_invert_torch,  # noqa: F401
                     _nb_quantiles_torch, philox4x32, sample_uniforms)

_last_backend: Optional[str] = None
_last_group_entry: Optional[str] = None     # the C entry the last hip ``group_sums`` ran


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
    """``t`` [B,H,N] or [P,B,H,N] as the kernels take it: rows contiguous and N apart (batch and path strides of its
    own are fine, ``runtime.rows_ok``), else a contiguous copy."""
    from . import runtime as rt

    return t if rt.rows_ok(t) else t.contiguous()


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


# ---------------------------------------------------------------------------------------------- quantiles and CDF
# ``hip``: k_nb_cdf / k_nb_quantile (csrc/quantile.hip).  ``torch``: the same continued fraction and the same bracketed
# search in fp64 torch ops (nbdist.py), so the functions run on CPU tensors.


def _check_levels(levels, who: str = "nb_quantiles", allow_empty: bool = False) -> List[float]:
    lv = [float(q) for q in levels]
    if not lv and not allow_empty:
        raise ValueError(f"{who}: no levels")
    for q in lv:
        if not 0.0 < q < 1.0:
            raise ValueError(f"{who}: level {q} is not strictly inside (0, 1)")
    return lv


def _use_hip(who: str, backend, eligible: bool, takes: str) -> bool:
    """Which backend a call with a ``backend`` argument runs: ``hip`` where it can unless ``"torch"`` is asked for;
    asking for ``"hip"`` where it cannot run is an error, as is any other name."""
    if backend not in (None, "hip", "torch"):
        raise ValueError(f"{who}: backend {backend!r} is not 'hip', 'torch' or None")
    if backend == "hip" and not eligible:
        raise ValueError(f"{who}: backend 'hip' takes {takes}")
    return eligible and backend != "torch"


def _calibration(valid, target, Q, lv):
    """``(coverage [Q], pinball [Q], den)`` of the quantiles ``Q`` [Q,B,H,N] at levels ``lv`` against ``target``
    [B,H,N] over the ``valid`` elements: the means of ``target <= Q`` and of ``max(q d, (q - 1) d)`` with
    ``d = target - Q``, and the fp32 count they were divided by (at least 1)."""
    w = valid.to(torch.float32)
    den = w.sum().clamp(min=1.0)
    zero = torch.zeros((), dtype=torch.float32, device=Q.device)
    yv = torch.where(valid, target, zero)
    Qv = torch.where(valid, Q, zero)
    diff = yv - Qv                                              # the levels stay Python scalars: no host-to-device copy
    pin = torch.stack([torch.maximum(q * diff[i], (q - 1.0) * diff[i]) for i, q in enumerate(lv)]) * w
    return ((yv <= Qv).to(torch.float32) * w).sum((1, 2, 3)) / den, pin.sum((1, 2, 3)) / den, den


def nb_cdf(y: torch.Tensor, rate: torch.Tensor, dispersion: torch.Tensor, eps: float = 1e-8) -> torch.Tensor:
    """``F(y)`` of the negative binomial ``(rate, dispersion)`` per element, fp32 [B,H,N]: ``I_p(r, floor(yc) + 1)``
    with the scorer's clamps (``yc = max(y, 0)``, ``alpha = max(dispersion, eps)``, ``mu = max(rate, eps)``,
    ``r = 1 / alpha``, ``p = 1 / (1 + alpha mu)``).  NaN where ``yc``, ``alpha`` or ``mu`` is not finite, and where
    ``floor(yc) >= 2^24``.  Never synchronises on the ``hip`` backend."""
    global _last_backend
    if _hip_eligible(y, rate, dispersion):
        from . import runtime as rt

        out = rt.nb_cdf(_rows(y), _rows(rate), _rows(dispersion), eps)
        _last_backend = "hip"
        return out
    if not (tuple(y.shape) == tuple(rate.shape) == tuple(dispersion.shape)):
        raise ValueError(f"nb_cdf takes y, rate, dispersion of one shape, got {tuple(y.shape)} {tuple(rate.shape)} "
                         f"{tuple(dispersion.shape)}")
    with torch.no_grad():
        F, _ = _nb_cdf_torch(y, rate, dispersion, eps)
    _last_backend = "torch"
    return F.to(torch.float32)


def nb_quantiles(rate: torch.Tensor, dispersion: torch.Tensor, levels, eps: float = 1e-8,
                 check: bool = False) -> torch.Tensor:
    """``Q(q)`` for every ``q`` of ``levels`` (floats strictly inside (0, 1), any order, any number: the kernel takes
    8 per launch): the smallest integer k >= 0 with ``F(k) >= q``, as fp32 [Q,B,H,N].  Supported answers are below
    2^24; an element beyond that is NaN and sets bit 1 of a device flag that only ``check=True`` reads (one
    synchronisation; raises ``ValueError``).  NaN, without the flag, where ``alpha`` or ``mu`` is not finite."""
    global _last_backend
    lv = _check_levels(levels)
    if _hip_eligible(rate, dispersion):
        from . import runtime as rt

        r, d = _rows(rate), _rows(dispersion)
        flag = torch.zeros(1, dtype=torch.int32, device=rate.device)
        out = torch.empty((len(lv),) + tuple(rate.shape), dtype=torch.float32, device=rate.device)
        for i in range(0, len(lv), NBQ_QMAX):
            rt.nb_quantiles(r, d, lv[i:i + NBQ_QMAX], eps, out=out[i:i + NBQ_QMAX], flag=flag)
        _last_backend = "hip"
    else:
        if tuple(rate.shape) != tuple(dispersion.shape):
            raise ValueError(f"nb_quantiles takes rate and dispersion of one shape, got {tuple(rate.shape)} "
                             f"{tuple(dispersion.shape)}")
        with torch.no_grad():
            out, flag = _nb_quantiles_torch(rate, dispersion, lv, eps)
        _last_backend = "torch"
    if check and int(flag.reshape(-1)[0]) & NBQ_FLAG_RANGE:
        raise ValueError("nb_quantiles: an element's quantile is outside the supported range [0, 2^24) (or its "
                         "search hit an iteration cap); that element is NaN")
    return out


def prediction_interval(rate: torch.Tensor, dispersion: torch.Tensor, coverage: float = 0.9, eps: float = 1e-8):
    """``(lo, hi)``: the ``(1 - coverage) / 2`` and ``(1 + coverage) / 2`` quantiles, each fp32 [B,H,N]."""
    c = float(coverage)
    if not 0.0 < c < 1.0:
        raise ValueError(f"prediction_interval: coverage {c} is not strictly inside (0, 1)")
    q = nb_quantiles(rate, dispersion, [(1.0 - c) / 2.0, (1.0 + c) / 2.0], eps)
    return q[0], q[1]


def interval_metrics(y: torch.Tensor, rate: torch.Tensor, dispersion: torch.Tensor, levels,
                     mask: torch.Tensor | None = None, eps: float = 1e-8) -> Dict[str, torch.Tensor]:
    """Calibration of the distribution over the valid elements (``negative_binomial_mask``; an element whose quantile
    or CDF came out NaN is dropped too), as tensors on ``y``'s device and without a host read: ``coverage`` [Q], the
    mean of ``y <= Q(q)``; ``pinball`` [Q], the mean of ``max(q (y - Q), (q - 1) (y - Q))``; ``pit_mean``, the mean
    of ``F(y)``; ``count``, the valid elements (int64)."""
    lv = _check_levels(levels)
    Q = nb_quantiles(rate, dispersion, lv, eps)
    F = nb_cdf(y, rate, dispersion, eps)
    valid = negative_binomial_mask(y, rate, dispersion, mask) & torch.isfinite(F) & torch.isfinite(Q).all(0)
    coverage, pinball, den = _calibration(valid, y.to(torch.float32), Q, lv)
    return {"coverage": coverage, "pinball": pinball, "pit_mean": torch.where(valid, F, F.new_zeros(())).sum() / den,
            "count": valid.sum()}


# --------------------------------------------------------------------------------------------------------- sampling
# ``hip``: k_nb_sample (csrc/sample.hip).  ``torch``: the same Philox in int64 ops and the same search at a level per
# element, started as the kernel starts it (nbdist.py).


def nb_sample(rate: torch.Tensor, dispersion: torch.Tensor, n_samples: int = 1, seed=0, offset: int = 0,
              eps: float = 1e-8, backend: Optional[str] = None, return_uniforms: bool = False,
              flag: Optional[torch.Tensor] = None):
    """``n_samples`` draws of the negative binomial ``(rate, dispersion)`` per element, fp32 [S,B,H,N], in
    ``nb_quantiles``' parameterisation: draw s of element e is ``Q(u[s, e])`` with ``u = sample_uniforms(S, rate.shape,
    seed, offset)``, so a draw depends on nothing but ``(seed, offset, e, s)`` and the element's distribution.
    ``seed``: a Python int or a one-element int64 / uint64 tensor on ``rate``'s device (read on the device: no
    synchronisation).  ``backend``: ``"hip"`` (k_nb_sample; fp32 [B,H,N] tensors on a ROCm device, nothing for autograd
    to record), ``"torch"`` (the same generator and search in torch ops, any device), or None: ``hip`` where it can
    run.  NaN where alpha or mu is not finite; an answer >= 2^24 is NaN too and ORs bit 1 into ``flag`` (one int32 on
    ``rate``'s device, optional).  ``return_uniforms``: ``(samples, u)``.  Never synchronises on the ``hip`` backend."""
    global _last_backend
    S = int(n_samples)
    if S < 1:
        raise ValueError(f"nb_sample: n_samples={n_samples}")
    if not 0 <= int(offset) <= _M32:
        raise ValueError(f"nb_sample: offset={offset} is not a 32-bit word")
    if tuple(rate.shape) != tuple(dispersion.shape) or rate.dim() != 3:
        raise ValueError(f"nb_sample takes rate and dispersion of one shape [B, H, N], got {tuple(rate.shape)} "
                         f"{tuple(dispersion.shape)}")
    if _use_hip("nb_sample", backend, _hip_eligible(rate, dispersion),
                "fp32 [B, H, N] tensors on one ROCm device, without autograd"):
        from . import runtime as rt

        out, _, u = rt.nb_sample(_rows(rate), _rows(dispersion), S, seed, offset, eps, flag=flag,
                                 want_uniforms=return_uniforms)
        _last_backend = "hip"
    else:
        with torch.no_grad():
            u = sample_uniforms(S, rate.shape, seed, offset, device=rate.device)
            out, bad = _nb_invert_torch(u, rate, dispersion, eps)
            if flag is not None:
                flag |= bad.to(flag.device)
        _last_backend = "torch"
    return (out, u) if return_uniforms else out


def path_quantiles(samples: torch.Tensor, levels, window: Optional[int] = None) -> torch.Tensor:
    """Quantiles over sample paths: ``samples`` [P,B,H,N] -> [Q,B,H',N].  With ``window``, every path is first summed
    over non-overlapping windows of ``window`` steps along H (``H' = H / window``; a ragged last window is an error).
    The quantile is the order statistic ``ceil(q P)`` of the P paths (the inverted-CDF definition: the smallest value
    whose empirical CDF reaches q), consistent with ``nb_quantiles``.  ``path_summary`` computes the same order
    statistics on the device in one pass, for window maxima too, with the mean and the CRPS beside them."""
    import math

    lv = _check_levels(levels)
    if samples.dim() != 4:
        raise ValueError(f"path_quantiles takes samples [P, B, H, N], got {tuple(samples.shape)}")
    P, B, H, N = samples.shape
    x = samples
    if window is not None:
        w = int(window)
        if w < 1 or H % w:
            raise ValueError(f"path_quantiles: window={window} does not divide H={H}")
        x = x.reshape(P, B, H // w, w, N).sum(3)
    ordered = torch.sort(x, dim=0).values
    rows = [min(max(math.ceil(q * P), 1), P) - 1 for q in lv]
    return ordered[rows]


# --------------------------------------------------------------------------------------------------- path summaries
# Per element (b, h', n): v[p] the window sum (fp64, rounded once to fp32) or window maximum (NaN stays) of path p,
# x(1) <= .. <= x(P) its sorted values (NaN last), quantile q = x(min(max(ceil(q P), 1), P)), mean = sum x / P and
#   crps = (A P - G) / P^2,  A = sum_p |x(p) - yw|,  G = sum_i (2 i - P - 1) x(i)
# the ensemble estimator (1/P) sum |v - yw| - (1/(2 P^2)) sum sum |v - v'|, every sum in fp64 and one rounding to fp32
# (include/flowtimes.h).  ``hip``: ftn_path_summary (csrc/paths.hip).  ``torch``: the same in torch ops, anywhere.
PATHS_MAX = 1024             # paths of one ftn_path_summary call (FTN_PATHS_MAX)


def _path_window(x: torch.Tensor, w: int, reduce: str) -> torch.Tensor:
    """``x`` [..., H, N] fp32 -> [..., H / w, N] fp32: window sums in fp64 rounded once, or window maxima."""
    H, N = x.shape[-2], x.shape[-1]
    g = x.reshape(*x.shape[:-2], H // w, w, N)
    if reduce == "max":
        return g.amax(-2)
    acc = torch.zeros(g.shape[:-2] + (N,), dtype=torch.float64, device=x.device)
    for j in range(w):                                          # ascending j, as the kernel adds
        acc = acc + g[..., j, :].double()
    return acc.to(torch.float32)


def _path_summary_torch(samples, ranks, w, reduce, y, want_sorted):
    P = samples.shape[0]
    xs = torch.sort(_path_window(samples, w, reduce), dim=0).values
    xd = xs.double()
    out = {"quantiles": xs[[r - 1 for r in ranks]] if ranks else xs[:0], "mean": (xd.sum(0) / P).to(torch.float32)}
    if y is not None:
        yw = _path_window(y, w, reduce).double()
        coef = (2.0 * torch.arange(1, P + 1, dtype=torch.float64, device=xs.device) - (P + 1)).view(P, 1, 1, 1)
        A, G = (xd - yw).abs().sum(0), (coef * xd).sum(0)
        out["crps"] = ((A * P - G) / float(P * P)).to(torch.float32)
    if want_sorted:
        out["sorted"] = xs
    return out


def path_summary(samples: torch.Tensor, levels=(), y: torch.Tensor | None = None, window: Optional[int] = None,
                 reduce: str = "sum", want_sorted: bool = False, backend: Optional[str] = None
                 ) -> Dict[str, torch.Tensor]:
    """Summaries of sample paths ``samples`` [P,B,H,N] per element of [B,H',N]: every path is first reduced over
    non-overlapping windows of ``window`` steps along H (``H' = H / window``; None: 1; a ragged last window is an
    error) by ``reduce``: ``"sum"`` or ``"max"``.  Returns fp32 tensors: ``quantiles`` [Q,B,H',N], the order statistic
    ``ceil(q P)`` of the P values for every ``q`` of ``levels`` (``path_quantiles``' definition; any number, none is
    fine); ``mean`` [B,H',N]; with ``y`` [B,H,N], ``crps`` [B,H',N], the sample CRPS of the P values against the same
    reduce of ``y`` (the plain ensemble estimator, 0 for P = 1 and y on the sample); with ``want_sorted``, ``sorted``
    [P,B,H',N].  NaN sorts last and makes mean and CRPS NaN.  ``backend``: ``"hip"`` (one ``ftn_path_summary`` launch
    per 8 levels; fp32 samples on a ROCm device, nothing for autograd to record, P <= 1024), ``"torch"`` (the same
    definitions in torch ops, any device; other dtypes are converted to fp32 first), or None: ``hip`` where it can
    run.  Never synchronises on the ``hip`` backend."""
    import math

    global _last_backend
    lv = _check_levels(levels, "path_summary", allow_empty=True)
    if reduce not in ("sum", "max"):
        raise ValueError(f"path_summary: reduce {reduce!r} is not 'sum' or 'max'")
    if not isinstance(samples, torch.Tensor) or samples.dim() != 4 or samples.numel() == 0:
        raise ValueError(f"path_summary takes samples [P, B, H, N], got "
                         f"{tuple(samples.shape) if isinstance(samples, torch.Tensor) else type(samples)}")
    P, B, H, N = samples.shape
    w = 1 if window is None else int(window)
    if w < 1 or H % w:
        raise ValueError(f"path_summary: window={window} does not divide H={H}")
    if y is not None and (not isinstance(y, torch.Tensor) or tuple(y.shape) != (B, H, N)):
        raise ValueError(f"path_summary: y must be [B, H, N] = {(B, H, N)}, got "
                         f"{tuple(y.shape) if isinstance(y, torch.Tensor) else type(y)}")
    ranks = [min(max(math.ceil(q * P), 1), P) for q in lv]
    eligible = (samples.is_cuda and samples.dtype == torch.float32 and P <= PATHS_MAX
                and not (torch.is_grad_enabled() and (samples.requires_grad or (y is not None and y.requires_grad))))
    if _use_hip("path_summary", backend, eligible,
                f"fp32 [P, B, H, N] samples on a ROCm device, without autograd, P <= {PATHS_MAX}"):
        from . import runtime as rt

        yk = None
        if y is not None:
            yk = _rows(y.detach().to(device=samples.device, dtype=torch.float32))
        res = rt.path_summary(_rows(samples.detach()), ranks, w, reduce, y=yk, want_mean=True,
                              want_sorted=want_sorted)
        if res["quantiles"] is None:
            res["quantiles"] = torch.empty((0, B, H // w, N), dtype=torch.float32, device=samples.device)
        out = {k: v for k, v in res.items() if v is not None}
        _last_backend = "hip"
    else:
        with torch.no_grad():
            yt = None if y is None else y.to(device=samples.device, dtype=torch.float32)
            out = _path_summary_torch(samples.to(torch.float32), ranks, w, reduce, yt, want_sorted)
        _last_backend = "torch"
    return out


def path_metrics(samples: torch.Tensor, y: torch.Tensor, levels, window: Optional[int] = None, reduce: str = "sum",
                 mask: torch.Tensor | None = None) -> Dict[str, torch.Tensor]:
    """``interval_metrics`` for sample paths: calibration and score of the paths' window sums or maxima against the
    same reduce ``yw`` of ``y`` [B,H,N], over the valid elements, as tensors on ``samples``' device and without a
    host read: ``coverage`` [Q], the mean of ``yw <= Q(q)``; ``pinball`` [Q], the mean of
    ``max(q (yw - Q), (q - 1) (yw - Q))``; ``crps``, the mean sample CRPS; ``count``, the valid elements (int64).
    An element is valid where ``yw``, its quantiles and its CRPS are finite and, with ``mask`` [B,H,N], every step
    of its window is inside the mask."""
    lv = _check_levels(levels, "path_metrics")
    s = path_summary(samples, lv, y, window, reduce)
    Q, crps = s["quantiles"], s["crps"]
    P, B, H, N = samples.shape
    w = 1 if window is None else int(window)
    yw = _path_window(y.detach().to(device=Q.device, dtype=torch.float32), w, reduce)
    valid = torch.isfinite(yw) & torch.isfinite(Q).all(0) & torch.isfinite(crps)
    if mask is not None:
        if tuple(mask.shape) != (B, H, N):
            raise ValueError(f"path_metrics: mask must be [B, H, N] = {(B, H, N)}, got {tuple(mask.shape)}")
        valid = valid & mask.to(device=Q.device).to(torch.bool).reshape(B, H // w, w, N).all(2)
    coverage, pinball, den = _calibration(valid, yw, Q, lv)
    return {"coverage": coverage, "pinball": pinball, "crps": torch.where(valid, crps, crps.new_zeros(())).sum() / den,
            "count": valid.sum()}


# ----------------------------------------------------------------------------------------------------- series groups
# out[.., g] = the sum of x[.., i] over the members i of group g, defined to the bit (include/flowtimes.h): the members
# in chunks of 32, a chunk's sum in fp64 left to right from +0.0, the chunk sums in ascending order in fp64, one
# rounding to fp32.  ``hip``: ftn_group_sum (csrc/groups.hip).  ``torch``: the same additions in torch ops, anywhere.
# GROUP_CHUNK, and GROUP_NMAX / GMAX / CHUNKS_MAX, the series, groups and chunks of one ftn_group_sum call: lib.py's.


def _store_key(series_id: str) -> str:
    """The reference's store of a series id ``"store_menu"`` (utils/metrics.py: ``c.split("_", 1)[0]``)."""
    return series_id.split("_", 1)[0]


class SeriesGroups:
    """Groups of series as member lists, built once on the host: ``names`` [G], ``n_series`` N, ``n_groups`` G, and
    the CSR ``order`` [M] / ``offsets`` [G+1] as int32 tensors on ``device`` (group g's members are
    ``order[offsets[g]:offsets[g+1]]``, in that order, which is the order ``group_sums`` adds them in).  A series may
    be in no group, in one or in several; an empty group is fine.  Rejected: an index outside 0..N-1, a series
    repeated inside one group, no group at all."""

    def __init__(self, members, n_series: int, names=None, device=None):
        N = int(n_series)
        if N < 1:
            raise ValueError(f"SeriesGroups: n_series={n_series} is not positive")
        lists = [[int(i) for i in m] for m in members]
        if not lists:
            raise ValueError("SeriesGroups: no group (G == 0)")
        for g, m in enumerate(lists):
            for i in m:
                if not 0 <= i < N:
                    raise ValueError(f"SeriesGroups: group {g} holds index {i} outside 0..{N - 1}")
            if len(set(m)) != len(m):
                raise ValueError(f"SeriesGroups: group {g} holds a series more than once (a duplicate)")
        self.names = [str(g) for g in range(len(lists))] if names is None else [str(n) for n in names]
        if len(self.names) != len(lists):
            raise ValueError(f"SeriesGroups: {len(self.names)} names for {len(lists)} groups")
        self.n_series, self.n_groups = N, len(lists)
        self.members = lists
        self.offsets_host = np.zeros(len(lists) + 1, dtype=np.int32)
        np.cumsum([len(m) for m in lists], out=self.offsets_host[1:])
        self.order_host = np.array([i for m in lists for i in m], dtype=np.int32).reshape(-1)
        self.n_chunks = sum((len(m) + GROUP_CHUNK - 1) // GROUP_CHUNK for m in lists)
        self.device = torch.device("cpu" if device is None else device)
        self.order = torch.from_numpy(self.order_host).to(self.device)
        self.offsets = torch.from_numpy(self.offsets_host).to(self.device)
        self._tables = None
        self._moved: Dict[torch.device, "SeriesGroups"] = {}

    @classmethod
    def from_ids(cls, ids, key=None, device=None) -> "SeriesGroups":
        """One group per distinct ``key(id)`` (default: the reference's store rule, the text before the first
        ``"_"``), the groups in first-appearance order as the reference's ``store_to_idx``, members ascending."""
        key = _store_key if key is None else key
        index: Dict[str, int] = {}
        members: List[List[int]] = []
        for i, s in enumerate(ids):
            k = key(s)
            if k not in index:
                index[k] = len(members)
                members.append([])
            members[index[k]].append(i)
        n = sum(len(m) for m in members)
        return cls(members, max(n, 1), list(index), device)

    @classmethod
    def from_labels(cls, labels, device=None) -> "SeriesGroups":
        """``labels`` int [N]: series n is in group ``labels[n]``, or in none where that is -1; G = max label + 1."""
        lab = np.asarray(labels.cpu() if isinstance(labels, torch.Tensor) else labels)
        if lab.ndim != 1 or lab.size == 0 or lab.dtype.kind not in "iu":
            raise ValueError("SeriesGroups.from_labels takes a non-empty integer vector [N]")
        if int(lab.min()) < -1:
            raise ValueError(f"SeriesGroups.from_labels: label {int(lab.min())} is below -1")
        G = int(lab.max()) + 1
        return cls([np.nonzero(lab == g)[0].tolist() for g in range(G)], lab.size, None, device)

    @classmethod
    def from_members(cls, members, names=None, n_series: Optional[int] = None, device=None) -> "SeriesGroups":
        """The general form: one list of series indices per group, overlap allowed.  ``n_series``: N (default: the
        largest index + 1)."""
        lists = [[int(i) for i in m] for m in members]
        if n_series is None:
            n_series = max([i for m in lists for i in m], default=0) + 1
        return cls(lists, n_series, names, device)

    def with_total(self, name: str = "total") -> "SeriesGroups":
        """These groups and one more that holds every series, in ascending index."""
        return SeriesGroups(self.members + [list(range(self.n_series))], self.n_series, self.names + [name],
                            self.device)

    def to(self, device) -> "SeriesGroups":
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device == self.device:
            return self
        if device not in self._moved:                           # one upload per device, whoever asks
            self._moved[device] = SeriesGroups(self.members, self.n_series, self.names, device)
        return self._moved[device]

    def sizes(self) -> List[int]:
        return [len(m) for m in self.members]

    def _torch_tables(self):
        """``(idx [C,32], cidx [G,K])`` on the device: the members of every chunk, padded with N (a zero column), and
        the chunks of every group, padded with C (a zero column)."""
        if self._tables is None:
            C, N = self.n_chunks, self.n_series
            idx = np.full((max(C, 1), GROUP_CHUNK), N, dtype=np.int64)
            per = [(len(m) + GROUP_CHUNK - 1) // GROUP_CHUNK for m in self.members]
            cidx = np.full((self.n_groups, max(max(per), 1)), C, dtype=np.int64)
            c = 0
            for g, m in enumerate(self.members):
                for k in range(per[g]):
                    part = m[k * GROUP_CHUNK:(k + 1) * GROUP_CHUNK]
                    idx[c, :len(part)] = part
                    cidx[g, k] = c
                    c += 1
            self._tables = (torch.from_numpy(idx[:C]).to(self.device), torch.from_numpy(cidx).to(self.device))
        return self._tables


def _group_sums_torch(x: torch.Tensor, groups: SeriesGroups) -> torch.Tensor:
    idx, cidx = groups._torch_tables()
    N, G, C = groups.n_series, groups.n_groups, groups.n_chunks
    rows = x.to(torch.float32).reshape(-1, N)
    R = rows.shape[0]
    xz = torch.cat([rows.double(), torch.zeros(R, 1, dtype=torch.float64, device=x.device)], 1)
    acc = torch.zeros(R, C, dtype=torch.float64, device=x.device)
    for j in range(GROUP_CHUNK):                                # left to right; a slot beyond the chunk adds +0.0
        acc = acc + xz[:, idx[:, j]]
    cz = torch.cat([acc, torch.zeros(R, 1, dtype=torch.float64, device=x.device)], 1)
    tot = torch.zeros(R, G, dtype=torch.float64, device=x.device)
    for k in range(cidx.shape[1]):                              # ascending chunk
        tot = tot + cz[:, cidx[:, k]]
    return tot.to(torch.float32).reshape(*x.shape[:-1], G)


def _group_rows(x: torch.Tensor) -> torch.Tensor:
    """``x`` [..., N] as [rows, N] with one row stride: a view where the leading dims collapse, else a copy."""
    N = x.shape[-1]
    if N > 1 and x.stride(-1) != 1:
        x = x.contiguous()
    try:
        v = x.view(-1, N)
    except RuntimeError:
        v = x.contiguous().view(-1, N)
    if v.shape[0] > 1 and v.stride(0) < N:                      # an expanded row
        v = v.contiguous()
    return v


def _group_slabs(x: torch.Tensor, axis: int) -> torch.Tensor:
    """``x`` as [outer, S, inner] around dim ``axis`` (the ``_group_rows`` policy on both sides of it): a view where
    the dims before ``axis`` collapse to one slab stride, the dims after it collapse with an innermost stride of 1,
    and neither members nor slabs overlap; else one copy to contiguous."""
    S = x.shape[axis]
    outer, inner = math.prod(x.shape[:axis]), math.prod(x.shape[axis + 1:])
    try:
        v = x.view(outer, S, inner)
    except RuntimeError:
        return x.contiguous().view(outer, S, inner)
    ms = v.stride(1) if S > 1 else inner
    if ((inner > 1 and v.stride(2) != 1) or (S > 1 and ms < inner) or (outer > 1 and v.stride(0) < S * ms)):
        v = x.contiguous().view(outer, S, inner)
    return v


def group_sums(x: torch.Tensor, groups: SeriesGroups, backend: Optional[str] = None, axis: int = -1) -> torch.Tensor:
    """Totals over groups of series: ``x`` [..., N] -> fp32 [..., G], ``out[.., g]`` the sum of ``x[.., i]`` over the
    members of group g in the order and precision stated above (exact for integer-valued x whose totals stay below
    2^24; NaN and inf reach only the groups that hold them; an empty group gives +0).  Works on sample paths
    [P,B,H,N] (``path_summary`` then applies to the totals), on ``rate`` (means add), on ``y`` and on 0/1 masks.
    ``backend``: ``"hip"`` (one ``ftn_group_sum`` launch; fp32 on a ROCm device, nothing for autograd to record,
    N <= 8192, at most 2048 groups and 2048 chunks of 32 members; leading dims that collapse to one row stride are
    passed as a view, anything else is copied), ``"torch"`` (the same additions in torch ops, any device, bit-equal;
    other dtypes are converted to fp32 first), or None: ``hip`` where it can run.  Never synchronises on ``hip``.

    ``axis``: the dim the series lie along (default: the last, all of the above unchanged).  Any other dim must hold
    ``groups.n_series`` members and the result has G in its place - the pipeline layout, one series per batch row:
    ``group_sums(samples[P,B,H,1], groups, axis=1)`` -> [P,G,H,1], to the same bits as the totals of the transposed
    copy.  On ``hip`` that is one ``ftn_group_sum_rows`` launch, with no limit on the number of members (groups and
    chunks as above): the dims before ``axis`` collapse to ``outer`` and the dims after it to ``inner``, and x is
    passed as a view when both collapses are views, the innermost stride is 1 and neither members nor slabs overlap;
    otherwise it is copied once to contiguous.  Where the dims after ``axis`` hold one element in all, the members
    are 1 apart and there are at most 8192 of them, that view is [outer, N] with N fastest and goes to
    ``ftn_group_sum`` instead (``ftn_group_sum_rows`` with one column a member would be an uncoalesced gather)."""
    global _last_backend, _last_group_entry
    if not isinstance(groups, SeriesGroups):
        raise ValueError(f"group_sums: groups must be a SeriesGroups, got {type(groups)}")
    if isinstance(x, torch.Tensor) and x.dim() >= 1:
        if not isinstance(axis, int) or not -x.dim() <= axis < x.dim():
            raise ValueError(f"group_sums: axis={axis!r} is not a dim of x {tuple(x.shape)}")
        axis %= x.dim()
    last = not isinstance(x, torch.Tensor) or x.dim() < 1 or axis == x.dim() - 1
    if last and (not isinstance(x, torch.Tensor) or x.dim() < 1 or x.shape[-1] != groups.n_series or x.numel() == 0):
        raise ValueError(f"group_sums takes x [..., N] with N = {groups.n_series} series, got "
                         f"{tuple(x.shape) if isinstance(x, torch.Tensor) else type(x)}")
    if not last and (x.shape[axis] != groups.n_series or x.numel() == 0):
        raise ValueError(f"group_sums: dim {axis} of x {tuple(x.shape)} must hold the {groups.n_series} series of the "
                         f"groups")
    eligible = (x.is_cuda and x.dtype == torch.float32 and not (torch.is_grad_enabled() and x.requires_grad)
                and (groups.n_series <= GROUP_NMAX or not last) and groups.n_groups <= GROUP_GMAX
                and groups.n_chunks <= GROUP_CHUNKS_MAX)
    use_hip = _use_hip("group_sums", backend, eligible,
                       f"fp32 [..., N] on a ROCm device, without autograd, N <= {GROUP_NMAX} along the last dim, at most "
                       f"{GROUP_GMAX} groups and {GROUP_CHUNKS_MAX} chunks of {GROUP_CHUNK} members")
    groups = groups.to(x.device)
    if use_hip:
        from . import runtime as rt

        if last:
            out = rt.group_sum(_group_rows(x.detach()), groups.order, groups.offsets, groups.offsets_host)
            out = out.view(*x.shape[:-1], groups.n_groups)
            _last_group_entry = "ftn_group_sum"
        else:
            v = _group_slabs(x.detach(), axis)
            outer, S, inner = v.shape
            if inner == 1 and S <= GROUP_NMAX and (S == 1 or v.stride(1) == 1):
                out = rt.group_sum(v[:, :, 0], groups.order, groups.offsets, groups.offsets_host)
                _last_group_entry = "ftn_group_sum"
            else:
                out = rt.group_sum_rows(v, groups.order, groups.offsets, groups.offsets_host)
                _last_group_entry = "ftn_group_sum_rows"
            out = out.view(*x.shape[:axis], groups.n_groups, *x.shape[axis + 1:])
        _last_backend = "hip"
    else:
        with torch.no_grad():
            if last:
                out = _group_sums_torch(x, groups)
            else:
                out = _group_sums_torch(x.movedim(axis, -1), groups).movedim(-1, axis).contiguous()
        _last_backend = "torch"
    return out


def _group_path_axis(who: str, samples, axis) -> int:
    """The dim of ``samples`` [P,B,H,N] the groups run along: 3 (series) or 1 (batch rows, the pipeline layout)."""
    if not isinstance(samples, torch.Tensor) or samples.dim() != 4:
        raise ValueError(f"{who} takes samples [P, B, H, N]")
    if axis in (3, -1):
        return 3
    if axis in (1, -3):
        return 1
    raise ValueError(f"{who}: axis={axis!r} is neither the series axis (3 or -1) nor the batch axis (1 or -3) of "
                     f"samples [P, B, H, N]")


def group_path_summary(samples: torch.Tensor, groups: SeriesGroups, levels=(), y: torch.Tensor | None = None,
                       window: Optional[int] = None, reduce: str = "sum", want_sorted: bool = False,
                       backend: Optional[str] = None, axis: int = -1) -> Dict[str, torch.Tensor]:
    """``path_summary`` of the group totals: ``samples`` [P,B,H,N] -> ``group_sums`` [P,B,H,G], summarised against
    ``group_sums(y)``.  The total over the group is taken first and the window reduce second, so ``reduce="max"``
    is the peak of a store's total, not the total of its items' peaks.  Returns [.., B, H', G] tensors.
    ``axis=1`` (or -3): the groups are sets of batch rows, ``groups.n_series == B`` - the pipeline layout, one series
    per row, ``samples`` [P,B,H,1] - and ``y`` [B,H,N] is totalled along dim 0; the results are [.., G, H', N]."""
    ax = _group_path_axis("group_path_summary", samples, axis)
    if y is not None and (not isinstance(y, torch.Tensor) or tuple(y.shape) != tuple(samples.shape[1:])):
        raise ValueError(f"group_path_summary: y must be [B, H, N] = {tuple(samples.shape[1:])}")
    totals = group_sums(samples, groups, backend, axis=ax)
    yt = None
    if y is not None:
        yt = group_sums(y.detach().to(device=samples.device, dtype=torch.float32), groups, backend, axis=ax - 1)
    return path_summary(totals, levels, yt, window, reduce, want_sorted, backend)


def group_path_metrics(samples: torch.Tensor, y: torch.Tensor, groups: SeriesGroups, levels,
                       window: Optional[int] = None, reduce: str = "sum", mask: torch.Tensor | None = None,
                       axis: int = -1) -> Dict[str, torch.Tensor]:
    """``path_metrics`` on the group totals of ``samples`` [P,B,H,N] and ``y`` [B,H,N].  With ``mask`` [B,H,N] an
    element (b, h', g) is valid only if every member series of g is inside the mask at every step of its window: the
    group total of the masked-out indicator is 0 there (a count, exact), formed on the device.
    ``axis=1`` (or -3): the groups are sets of batch rows (``groups.n_series == B``); ``y`` and ``mask`` are totalled
    along dim 0 and an element (g, h', n) is valid only if every member row is inside the mask."""
    ax = _group_path_axis("group_path_metrics", samples, axis)
    if not isinstance(y, torch.Tensor) or tuple(y.shape) != tuple(samples.shape[1:]):
        raise ValueError(f"group_path_metrics: y must be [B, H, N] = {tuple(samples.shape[1:])}")
    if mask is not None and tuple(mask.shape) != tuple(y.shape):
        raise ValueError(f"group_path_metrics: mask must be [B, H, N] = {tuple(y.shape)}, got {tuple(mask.shape)}")
    totals = group_sums(samples, groups, axis=ax)
    yt = group_sums(y.detach().to(device=samples.device, dtype=torch.float32), groups, axis=ax - 1)
    gmask = None
    if mask is not None:
        outside = (~mask.to(device=samples.device).to(torch.bool)).to(torch.float32)
        gmask = group_sums(outside, groups, axis=ax - 1) == 0
    return path_metrics(totals, yt, levels, window, reduce, gmask)
