"""Table preparation on the device: static features, scalers, their transform and the inverse of a forecast.

What the reference does to the wide table ``[T, N]`` between the CSV and the loader, and to the forecast after the
model, without host arithmetic: ``series_features`` (``compute_series_features``, utils/static_features.py:17-103),
``SeriesScaler.fit`` (``fit_series_scaler``, utils/io.py:548-597, after ``clip_negative``, train.py:834),
``SeriesScaler.transform`` (``_transform_dataframe``, train.py:569-592) and ``SeriesScaler.inverse``
(``inverse_transform`` and the clip at 0, utils/io.py:600-621, predict.py:959-961).  ``min_sigma`` is the variability
summary behind the dispersion floor (``_masked_std``, train.py:447-566).  ``holdout_rows`` and ``rolling_rows`` are the
row ranges of data/split.py:7-33: a fold is a row slice of the device table, passed in place.
Calendar features, CSV and schema I/O, pivoting and pickled artefacts stay on the host.

Backends: ``torch`` is the reference's numpy restated line by line on CPU tensors (the reductions run in numpy itself,
on the tensors' memory, so that the order of every fp32 sum is the reference's) and is the definition; ``hip`` is
csrc/table.hip (``ftn_table_moments``, ``ftn_table_spectrum``, ``ftn_table_features``, ``ftn_table_scaler``,
``ftn_table_affine``) for fp32 tensors on a ROCm device.  ``backend=None`` takes ``hip`` for a ROCm tensor and ``torch``
for a CPU tensor; a ROCm input takes the torch path only when it is asked for by name.  ``_last_backend`` records which
ran last (``SeriesScaler.fit(..., "none")`` runs neither and leaves the record alone).  The mask is validity
(``> 0``); the HIP backend never uses the value of an element that is masked out, sums in fp64 and rounds once
(DESIGN.md section 8 lists the deviations).
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np
import torch

FEATURE_NAMES = ("mean", "std", "diff_std", "seasonal_strength", "dominant_period")
METHODS = ("zscore", "minmax", "none")
_F32_EPS = np.float32(1e-6)

_last_backend: Optional[str] = None


def _ran(backend: str) -> None:
    global _last_backend
    _last_backend = backend


def _table(v, name: str, device=None) -> torch.Tensor:
    """``v`` as an fp32 ``[T, N]`` tensor with contiguous rows; an fp32 tensor that already is one is kept as the view
    it is (a row or column slice of a device table stays in place)."""
    t = v if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(v)))
    t = t.to(device=device if device is not None else t.device, dtype=torch.float32)
    if t.dim() != 2:
        raise ValueError(f"{name} must be a [T, N] table, got {tuple(t.shape)}")
    if t.shape[1] > 1 and t.stride(1) != 1:
        t = t.contiguous()
    return t


def _backend(t: torch.Tensor, backend: Optional[str]) -> str:
    if backend not in (None, "hip", "torch"):
        raise ValueError(f"backend {backend!r} is not 'hip', 'torch' or None")
    if backend == "hip" and not t.is_cuda:
        raise ValueError("backend 'hip' takes tensors on a ROCm device")
    return backend if backend is not None else ("hip" if t.is_cuda else "torch")


def _safe_divide(numer: np.ndarray, denom: np.ndarray) -> np.ndarray:
    # utils/static_features.py:9-14
    denom_safe = np.maximum(denom.astype(np.float32, copy=False), _F32_EPS)
    return (numer.astype(np.float32, copy=False) / denom_safe).astype(np.float32, copy=False)


def _features_numpy(values: np.ndarray, mask: np.ndarray) -> np.ndarray:
    """utils/static_features.py:36-103 on fp32 arrays, line by line."""
    time_steps, num_series = values.shape
    if num_series == 0:                                                              # :48-49
        return np.zeros((0, len(FEATURE_NAMES)), dtype=np.float32)
    counts = mask.sum(axis=0, dtype=np.float32)                                      # :51
    sum_vals = (values * mask).sum(axis=0, dtype=np.float32)                         # :52
    mean = _safe_divide(sum_vals, counts)                                            # :53
    centered = (values - mean[np.newaxis, :]) * mask                                 # :55
    var = _safe_divide((centered * centered).sum(axis=0, dtype=np.float32),          # :56-59
                       np.maximum(counts, np.float32(1.0)))
    std = np.sqrt(np.clip(var, 0.0, None)).astype(np.float32)                        # :60
    if time_steps > 1:                                                               # :62-73
        diffs = values[1:, :] - values[:-1, :]
        diff_mask = mask[1:, :] * mask[:-1, :]
        diff_counts = diff_mask.sum(axis=0, dtype=np.float32)
        diff_sum = (diffs * diff_mask).sum(axis=0, dtype=np.float32)
        diff_mean = _safe_divide(diff_sum, diff_counts)
        diff_centered = (diffs - diff_mean[np.newaxis, :]) * diff_mask
        diff_var = _safe_divide((diff_centered * diff_centered).sum(axis=0, dtype=np.float32),
                                np.maximum(diff_counts, np.float32(1.0)))
        diff_std = np.sqrt(np.clip(diff_var, 0.0, None)).astype(np.float32)
    else:                                                                            # :74-75
        diff_std = np.zeros(num_series, dtype=np.float32)
    seasonal_strength = np.zeros(num_series, dtype=np.float32)                       # :93-98
    dominant_period = np.zeros(num_series, dtype=np.float32)
    if time_steps > 1:                                                               # :77-92
        demeaned = np.where(mask > 0.0, values - mean[np.newaxis, :], 0.0)
        fft_vals = np.fft.rfft(demeaned, axis=0)
        power = np.abs(fft_vals) ** 2
        if power.shape[0] > 1:
            power_no_dc = power[1:, :]
            peak_indices = np.argmax(power_no_dc, axis=0)
            cols = np.arange(num_series)
            peak_power = power_no_dc[peak_indices, cols]
            total_power = power_no_dc.sum(axis=0)
            seasonal_strength = _safe_divide(peak_power, total_power)
            dominant_period = np.where(total_power > _F32_EPS,
                                       (time_steps / np.maximum(peak_indices + 1, 1)).astype(np.float32),
                                       0.0).astype(np.float32)
    return np.stack([mean, std, diff_std, seasonal_strength, dominant_period], axis=1).astype(np.float32, copy=False)


def series_features(values, mask=None, backend: Optional[str] = None) -> torch.Tensor:
    """The reference's per-series static features ``[N, 5]`` fp32 (``FEATURE_NAMES``) of the wide table ``values``
    [T, N] with validity ``mask`` [T, N] (0/1; None: every element counts), on the table's device.  Both may be row
    and column slices of a larger table; they are read in place."""
    X = _table(values, "values")
    M = None if mask is None else _table(mask, "mask", X.device)
    if M is not None and M.shape != X.shape:
        raise ValueError("values and mask must have the same shape")
    be = _backend(X, backend)
    if be == "hip":
        from . import runtime as rt

        T, N = X.shape
        if N == 0:
            out = torch.zeros(0, 5, dtype=torch.float32, device=X.device)
        elif T == 0:
            raise ValueError("values has no rows")
        else:
            stats = rt.table_moments(X, M, diffs=True)
            f_peak, peak, total = rt.table_spectrum(X, stats[2].to(torch.float32), M)
            out = rt.table_features(stats, f_peak, peak, total, T)
    else:
        v = X.detach().cpu().numpy()
        m = np.ones_like(v) if M is None else M.detach().cpu().numpy()
        out = torch.from_numpy(_features_numpy(v, m)).to(X.device)
    _ran(be)
    return out


MIN_SIGMA_METHODS = ("global", "per_series_median")


def _masked_std_numpy(values: np.ndarray, mask: Optional[np.ndarray], method: str):
    """train.py:472-564 for one table, line by line: ``(std, per-series std)``; the per-series vector also for
    ``"global"`` (the reference returns None there)."""
    n_series = values.shape[1]
    per_series = np.zeros(n_series, dtype=np.float64)
    if values.size == 0:                                                             # :482, :512
        return 0.0, per_series
    mask_bool = np.ones(values.shape, dtype=bool) if mask is None else mask > 0.0    # :487, :521-526
    if not np.any(mask_bool):                                                        # :488, :527
        return 0.0, per_series
    arr64 = values.astype(np.float64, copy=False)
    mask_float = mask_bool.astype(np.float64, copy=False)
    per_sum = (arr64 * mask_float).sum(axis=0)                                       # :541-543
    per_sum_sq = (np.square(arr64) * mask_float).sum(axis=0)
    per_count = mask_float.sum(axis=0)
    valid_series = per_count > 0.0                                                   # :548-560
    means = np.zeros_like(per_sum)
    means[valid_series] = per_sum[valid_series] / per_count[valid_series]
    variances = np.zeros_like(per_sum)
    variances[valid_series] = np.maximum(per_sum_sq[valid_series] / per_count[valid_series] - means[valid_series] ** 2,
                                         0.0)
    per_series[valid_series] = np.sqrt(variances[valid_series])
    if method == "per_series_median":
        return float(np.median(per_series[valid_series])), per_series                # :561-564
    values64 = arr64[mask_bool]                                                      # :490-503
    total, total_sq, count = float(values64.sum()), float(np.square(values64).sum()), int(values64.size)
    mean = total / count
    return float(np.sqrt(max(total_sq / count - mean * mean, 0.0))), per_series


def min_sigma(values, mask=None, method: str = "global", backend: Optional[str] = None):
    """The reference's variability summary behind the dispersion floor (``_masked_std``, train.py:447-566) of the wide
    table ``values`` [T, N] with validity ``mask`` (``> 0``; None: every element counts): ``(std, per_series)``, a
    0-dim fp64 tensor and the per-series standard deviations fp64 ``[N]`` (0 for a series without a valid point), on
    the table's device.  ``method``: ``"global"``, one standard deviation over all valid points, or
    ``"per_series_median"``, the median of the per-series ones over the series that have a valid point.  The floor
    itself is the caller's ``max(min_sigma, std * scale)`` (train.py:990-1001), and ``per_series * scale`` under the
    same maximum refreshes ``min_sigma_vector``.  ``hip``: ``ftn_table_moments`` and a few torch ops on its [6, N]
    statistics, no synchronisation.  Its centred sums square differences that were formed in fp32, so a standard
    deviation is within ``2^-24`` relative of the reference's fp64 value (which subtracts ``mean^2`` from the mean
    square)."""
    if method not in MIN_SIGMA_METHODS:
        raise ValueError(f"Unsupported min_sigma_method {method!r}. Expected 'global' or 'per_series_median'.")
    X = _table(values, "values")
    M = None if mask is None else _table(mask, "mask", X.device)
    if M is not None and M.shape != X.shape:
        raise ValueError("values and mask must have the same shape")
    be = _backend(X, backend)
    T, N = X.shape
    if be == "torch" or T == 0 or N == 0:
        std, per = _masked_std_numpy(X.detach().cpu().numpy(), None if M is None else M.detach().cpu().numpy(), method)
        out = torch.tensor(std, dtype=torch.float64, device=X.device), torch.from_numpy(per).to(X.device)
    else:
        from . import runtime as rt

        count, total, mean32, css = rt.table_moments(X, M)[:4]
        has = count > 0
        safe = torch.clamp(count, min=1.0)
        zero = torch.zeros_like(css)
        mean = torch.where(has, total / safe, zero)
        # css is centred on the fp32 mean: sum (v - m32)^2 = sum (v - m)^2 + count (m - m32)^2
        m2 = torch.where(has, torch.clamp(css - count * (mean - mean32) ** 2, min=0.0), zero)
        per = torch.sqrt(m2 / safe)
        if method == "global":
            n = torch.clamp(count.sum(), min=1.0)
            centre = torch.where(has, total, zero).sum() / n
            std = torch.sqrt((m2.sum() + (count * (mean - centre) ** 2).sum()) / n)
        else:                                                   # np.median over the k valid series, k on the device
            ranked = torch.sort(torch.where(has, per, torch.full_like(per, float("inf")))).values
            k = has.sum()
            mid = torch.stack([torch.clamp(k - 1, min=0) // 2, k // 2])
            std = torch.where(k > 0, ranked[mid].mean(), torch.zeros((), dtype=per.dtype, device=per.device))
        out = std, per
    _ran(be)
    return out


def _slice_rows(T: int, sl: slice) -> Tuple[int, int]:
    start, stop, _ = sl.indices(int(T))
    return start, max(start, stop)


def holdout_rows(T: int, holdout: int) -> Tuple[Tuple[int, int], Tuple[int, int]]:
    """``((train start, train end), (val start, val end))`` of ``make_holdout_slices`` (data/split.py:7-11): the rows
    ``iloc[:-holdout]`` and ``iloc[-holdout:]`` of a table of ``T`` rows."""
    holdout = int(holdout)
    if holdout <= 0:
        raise ValueError("holdout must be positive")
    return _slice_rows(T, slice(None, -holdout)), _slice_rows(T, slice(-holdout, None))


def rolling_rows(T: int, folds: int, step: int, val_len: int) -> List[Tuple[Tuple[int, int], Tuple[int, int]]]:
    """The ``(train rows, val rows)`` ranges ``make_rolling_slices`` yields (data/split.py:14-33), fold by fold from
    the tail, stopping at the first fold with an empty side."""
    out = []
    end = int(T)
    for k in range(int(folds)):
        val_end = end - k * int(step)
        val_start = max(0, val_end - int(val_len))
        trn, val = _slice_rows(T, slice(None, val_start)), _slice_rows(T, slice(val_start, val_end))
        if val[1] - val[0] == 0 or trn[1] - trn[0] == 0:
            break
        out.append((trn, val))
    return out


def _affine_torch(x: torch.Tensor, loc, scale, axis: int, series, inverse: bool, clip: bool, out):
    axis = axis % x.dim()
    S = x.shape[axis]
    idx = torch.arange(S, device=x.device) if series is None else series.to(x.device).clamp(0, loc.numel() - 1)
    shape = [1] * x.dim()
    shape[axis] = S
    l, s = loc[idx].reshape(shape), scale[idx].reshape(shape)
    zero = torch.zeros((), dtype=x.dtype, device=x.device)
    if inverse:
        r = x * s                                               # two roundings, as numpy's a * sd + mu
        r = r + l
        r = torch.where(r < 0, zero, r) if clip else r
    else:
        v = torch.where(x < 0, zero, x) if clip else x
        r = (v - l) / s
    if out is None:
        return r
    out.copy_(r)
    return out


class SeriesScaler:
    """The reference's series scaler with its state on the table's device: ``loc`` [N] and ``scale`` [N] fp32, so that
    ``transform`` is ``(x - loc) / scale`` and ``inverse`` is ``x * inv_scale + loc``, and the reference's pairs
    fp32 [2, N] - (mean, std) for ``zscore``, (min, max) for ``minmax`` - which ``pairs()`` hands back.  ``inv_scale``
    is ``scale`` except for a loaded zscore pair with std 0, where the reference divides by 1 and multiplies by 0."""

    def __init__(self, method: str, loc: torch.Tensor, scale: torch.Tensor, pair_rows: Optional[torch.Tensor],
                 per_series: bool = True, eps: float = 1e-8, inv_scale: Optional[torch.Tensor] = None) -> None:
        if method not in METHODS:
            raise ValueError(f"method {method!r} is not one of {METHODS}")
        self.method, self.per_series, self.eps = method, bool(per_series), float(eps)
        self.loc, self.scale, self._pairs = loc, scale, pair_rows
        self.inv_scale = scale if inv_scale is None else inv_scale

    @property
    def n_series(self) -> int:
        return int(self.loc.numel())

    @property
    def device(self) -> torch.device:
        return self.loc.device

    @classmethod
    def fit(cls, values, method: str = "zscore", per_series: bool = True, eps: float = 1e-8,
            clip_negative: bool = False, backend: Optional[str] = None) -> "SeriesScaler":
        """``fit_series_scaler`` on the rows of ``values`` [T, N] (pass the training rows: a row slice of the device
        table).  No mask, as in the reference.  ``clip_negative``: every value is read as ``max(v, 0)``
        (train.py:834); the clipped table is never written."""
        if method not in METHODS:
            raise ValueError(f"method {method!r} is not one of {METHODS}")
        X = _table(values, "values")
        T, N = X.shape
        if T < 1 or N < 1:
            raise ValueError(f"values must hold at least one row and one series, got {tuple(X.shape)}")
        be = _backend(X, backend)
        if method == "none":                                    # io.py:562-563; nothing runs: _last_backend keeps its record
            return cls(method, torch.zeros(N, dtype=torch.float32, device=X.device),
                       torch.ones(N, dtype=torch.float32, device=X.device), None, per_series, eps)
        if be == "hip":
            from . import runtime as rt

            stats = rt.table_moments(X, None, clip=clip_negative)
            loc, scale, pair_rows = rt.table_scaler(stats, method, per_series, eps)
        else:
            x = X.detach().cpu().numpy().astype(np.float32)                          # io.py:565
            if clip_negative:
                x = np.maximum(x, np.float32(0.0))                                   # train.py:835
            if per_series:
                if method == "zscore":                                               # io.py:567-573
                    a = np.mean(x, axis=0)
                    b = np.std(x, axis=0)
                    b = np.where(b < eps, 1.0, b)
                    sc = b
                else:                                                                # io.py:574-580
                    a = np.min(x, axis=0)
                    b = np.max(x, axis=0)
                    sc = np.where((b - a) < eps, 1.0, (b - a))
            else:
                if method == "zscore":                                               # io.py:583-589
                    mu = float(np.mean(x))
                    sd = float(np.std(x))
                    sd = sd if sd >= eps else 1.0
                    a, b, sc = np.full(N, mu), np.full(N, sd), np.full(N, sd)
                else:                                                                # io.py:590-596
                    mn = float(np.min(x))
                    mx = float(np.max(x))
                    rng = (mx - mn) if (mx - mn) >= eps else 1.0
                    a, b, sc = np.full(N, mn), np.full(N, mx), np.full(N, rng)
            to = lambda v: torch.from_numpy(np.ascontiguousarray(np.asarray(v, dtype=np.float32))).to(X.device)
            loc, scale, pair_rows = to(a), to(sc), to(np.stack([a, b]))
        _ran(be)
        return cls(method, loc, scale, pair_rows, per_series, eps)

    @classmethod
    def from_pairs(cls, method: str, pairs, ids=None, device=None) -> "SeriesScaler":
        """A scaler the reference fitted: ``pairs`` is its dict ``{id: (a, b)}`` (in the order of ``ids``, default the
        dict's own) or an array ``[N, 2]``.  ``loc`` and ``scale`` follow ``_transform_dataframe`` (train.py:582-589):
        zscore divides by ``std`` unless it is 0, minmax by ``max - min`` (formed in fp64) unless it is 0."""
        if method not in ("zscore", "minmax"):
            raise ValueError(f"from_pairs: method {method!r} is not 'zscore' or 'minmax'")
        if isinstance(pairs, dict):
            keys = list(pairs) if ids is None else list(ids)
            arr = np.array([pairs[k] for k in keys], dtype=np.float64).reshape(-1, 2)
        else:
            arr = np.asarray(pairs, dtype=np.float64)
        if arr.ndim != 2 or arr.shape[1] != 2 or arr.shape[0] < 1:
            raise ValueError(f"from_pairs: pairs must be [N, 2], got {arr.shape}")
        a, b = arr[:, 0], arr[:, 1]
        if method == "zscore":
            sc = np.where(b != 0, b, 1.0)                                            # train.py:584
            inv = b                                                                  # io.py:613-614
        else:
            rng = b - a
            sc = np.where(rng != 0, rng, 1.0)                                        # train.py:588, io.py:617
            inv = sc
        if device is None:
            device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
        to = lambda v: torch.from_numpy(np.ascontiguousarray(v.astype(np.float32))).to(device)
        return cls(method, to(a), to(sc), to(np.stack([a, b])), True, 0.0, inv_scale=to(inv))

    def pairs(self) -> Optional[np.ndarray]:
        """The reference's pairs as a host array ``[N, 2]`` fp64 (synchronises); None for method ``none``."""
        if self._pairs is None:
            return None
        return self._pairs.detach().cpu().numpy().astype(np.float64).T.copy()

    def _apply(self, x, axis, series, inverse, clip, out, backend):
        if not isinstance(x, torch.Tensor):
            x = torch.as_tensor(np.asarray(x), dtype=torch.float32).to(self.device)
        if x.dtype != torch.float32:
            x = x.to(torch.float32)
        if x.device != self.device:
            raise ValueError(f"the scaler lives on {self.device}, the tensor on {x.device}")
        if x.dim() < 1:
            raise ValueError("the tensor needs at least one dimension")
        if series is not None:
            on_device = isinstance(series, torch.Tensor) and series.device.type != "cpu"
            series = torch.as_tensor(series, dtype=torch.int64)
            if series.shape != (x.shape[axis],):
                raise ValueError(f"series must map the {x.shape[axis]} positions along axis {axis}")
            if not on_device and series.numel() and (int(series.min()) < 0 or int(series.max()) >= self.n_series):
                raise ValueError(f"series holds a column outside 0..{self.n_series - 1}")    # host data: checked here
            series = series.to(self.device).contiguous()
        elif x.shape[axis] != self.n_series:
            raise ValueError(f"{x.shape[axis]} series along axis {axis}, the scaler holds {self.n_series}")
        be = _backend(x, backend)
        sc = self.inv_scale if inverse else self.scale
        if be == "hip":
            from . import runtime as rt

            res = rt.table_affine(x, self.loc, sc, axis=axis, series=series, inverse=inverse, clip=clip, out=out)
        else:
            res = _affine_torch(x, self.loc, sc, axis, series, inverse, clip, out)
        _ran(be)
        return res

    def transform(self, values, out: Optional[torch.Tensor] = None, clip_negative: bool = False,
                  backend: Optional[str] = None) -> torch.Tensor:
        """``(x - loc) / scale`` in fp32 with the series along the last axis; ``clip_negative``: of ``max(x, 0)``.
        ``out`` may be ``values`` itself or a caller-owned buffer of its shape."""
        return self._apply(values, -1, None, False, clip_negative, out, backend)

    def inverse(self, pred, axis: int = -1, series=None, clip: bool = True, out: Optional[torch.Tensor] = None,
                backend: Optional[str] = None) -> torch.Tensor:
        """``x * scale + loc``, then ``max(., 0)`` when ``clip``, with the series along ``axis``.  ``series``: an int64
        map from a position along ``axis`` to the table's column - the pipeline layout ``[B, H, 1]``, where a series is
        a batch row, takes ``axis=0, series=ids_of_rows`` (the convention of ``group_sums(..., axis=)``).  A map given
        as host data (a list, an array, a CPU tensor) is validated and an entry outside ``0 .. N - 1`` is an error; a
        map that already lives on the device is not read back: both backends clamp its entries to ``0 .. N - 1`` when
        they use them, so a wrong id there yields the numbers of another series, never an out-of-bounds read."""
        return self._apply(pred, axis, series, True, clip, out, backend)
