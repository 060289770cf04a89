"""Sliding windows formed on the device: the batches of a rolling-origin backtest without a host loader.

``DeviceWindows`` holds the wide table ``[T, N]`` (values, validity mask, time features, statics, ids) on the device
once and forms every batch that the reference's ``SlidingWindowDataset`` (data/dataset.py:29-204) behind a
``DataLoader(shuffle=False, drop_last=False)`` would yield - the same item order, shapes, dtypes and bits - with one
``ftn_window_batch`` launch (csrc/windows.hip) and no host synchronisation, so
``score.eval_metrics(model, DeviceWindows(...), ...)`` is a whole backtest whose only synchronisation is the scorer's
``result()``.  The training augmentations, calendar-feature construction, scalers and shuffling are not part of it
(DESIGN.md section 8).

``layout="series"`` is the reference's: an item is one series of one window, item ``k`` = window ``k // N``, series
``k % N``.  ``layout="wide"`` is this project's ``[B, L, N]`` layout: an item is one window with all its series.

Backends: ``hip`` for fp32 tables on a ROCm device, a ``torch`` composition (index arithmetic and advanced indexing,
no Python loop over items) anywhere; both give the same bits.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch

LAYOUTS = ("series", "wide")
# The backend ``backend=None`` takes for a ROCm table, per layout (DESIGN.md section 4 "Device windows": HIP is the
# default of a layout only where it was at or below the torch composition at every measured shape of that layout).
DEFAULT_BACKEND = {"series": "hip", "wide": "hip"}


def _as_tensor(v, dtype, device) -> torch.Tensor:
    """``v`` (tensor or array-like) as a tensor of ``dtype`` on ``device`` with contiguous elements in its last dim;
    a tensor that already is one is kept as it is, so a row or column slice of a device table stays a view."""
    t = v if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(v)))
    t = t.to(device=device, dtype=dtype)
    if t.dim() >= 1 and t.shape[-1] > 1 and t.stride(-1) != 1:
        t = t.contiguous()
    return t


class _Part:
    """One table with its windows: what one ``SlidingWindowDataset`` holds."""

    def __init__(self, wide_values, input_len, pred_len, mode, recursive_pred_len, stride, valid_mask, series_static,
                 series_ids, time_features, device) -> None:
        if mode not in ("direct", "recursive"):
            raise ValueError(f"mode {mode!r} is not 'direct' or 'recursive'")
        if device is None:
            if isinstance(wide_values, torch.Tensor):
                device = wide_values.device
            else:
                device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
        X = _as_tensor(wide_values, torch.float32, torch.device(device))
        self.device = X.device                                  # with its index: "cuda" becomes "cuda:0"
        if X.dim() != 2:
            raise ValueError(f"wide_values must be a [T, N] table, got {tuple(X.shape)}")
        if valid_mask is not None and tuple(np.shape(valid_mask)) != tuple(X.shape):
            raise ValueError("valid_mask must match wide_values shape")
        self.X = X
        self.M = None if valid_mask is None else _as_tensor(valid_mask, torch.float32, self.device)
        self.T, self.N = X.shape
        if self.N <= 0:
            raise ValueError("wide_values must contain at least one series column")
        self.L = int(input_len)
        self.H = int(pred_len) if mode == "direct" else int(recursive_pred_len if recursive_pred_len is not None else 1)
        if self.L < 1 or self.H < 1:
            raise ValueError(f"input_len={self.L} and the target length {self.H} must be positive")
        max_start = self.T - self.L - self.H
        step = max(1, int(stride))
        self.starts_host = (np.zeros(0, dtype=np.int32) if max_start < 0
                            else np.ascontiguousarray(np.arange(0, max_start + 1, step, dtype=np.int64).astype(np.int32)))
        self.W = int(self.starts_host.size)
        self.starts = torch.from_numpy(self.starts_host).to(self.device)
        self.marks = None
        if time_features is not None:
            shape = tuple(np.shape(time_features))
            if len(shape) == 0 or shape[0] != self.T:
                raise ValueError("time_features must align with the temporal dimension of wide_values")
            if len(shape) > 2:
                raise ValueError("time_features must be a 2D array of shape [T, F]")
            feats = _as_tensor(time_features, torch.float32, self.device)
            feats = feats.reshape(-1, 1) if feats.dim() == 1 else feats
            self.marks = feats if feats.shape[1] > 0 else None
        self.F = 0 if self.marks is None else int(self.marks.shape[1])
        self.statics = None
        if series_static is not None:
            st = _as_tensor(series_static, torch.float32, self.device)
            st = st.reshape(-1, 1) if st.dim() == 1 else st
            if st.dim() != 2 or st.shape[0] != self.N:
                raise ValueError("series_static must have shape [num_series, num_features]")
            self.statics = st.contiguous()
        self.Fs = 0 if self.statics is None else int(self.statics.shape[1])
        self.ids = None
        if series_ids is not None:
            ids = series_ids if isinstance(series_ids, torch.Tensor) else torch.from_numpy(np.asarray(series_ids))
            if ids.dim() != 1:
                raise ValueError("series_ids must be a 1D sequence")
            if ids.shape[0] != self.N:
                raise ValueError("series_ids length must match number of series")
            self.ids = ids.to(device=self.device, dtype=torch.int64).contiguous()

    def items(self, layout: str) -> int:
        return self.W * self.N if layout == "series" else self.W

    def signature(self):
        return (self.L, self.H, self.F, self.statics is not None, self.Fs, self.ids is not None)


class DeviceWindows:
    """The batches of ``DataLoader(SlidingWindowDataset(wide_values, input_len, pred_len, mode, ...),
    batch_size, shuffle=False, drop_last=False)`` formed on ``device``.

    ``wide_values`` [T, N], ``valid_mask`` [T, N], ``time_features`` [T, F] (precomputed; or [T]), ``series_static``
    [N, Fs] (or [N]) and ``series_ids`` [N] are tensors or arrays; they are converted once (fp32, ids int64) and kept
    on ``device`` (default: the device of a tensor ``wide_values``; for an array the first ROCm device, else the CPU).
    An fp32 device tensor is kept as the view it is.  ``H = pred_len`` in direct mode, else ``recursive_pred_len or 1``;
    the window starts are ``arange(0, T - L - H + 1, max(1, stride))``, none when ``T < L + H``.

    ``len(w)`` batches, ``w.n_items`` items, ``w.n_windows`` windows, ``w.starts`` their start rows.  ``w.batch(i)`` is
    the i-th batch tuple, ``iter(w)`` yields them in order:

    * ``layout="series"``: ``(x [B, L, 1], y [B, H, 1], mask [B, H, 1], x_mark [B, L, F], y_mark [B, H, F]
      [, static [B, 1, Fs]][, ids [B, 1] int64])`` - what default collation makes of the dataset's items; the marks
      are fp32 ``[B, 0]`` without time features, and the last batch is short.
    * ``layout="wide"``: ``(x [B, L, N], y [B, H, N], mask [B, H, N], x_mark [B, L, F], y_mark [B, H, F]
      [, static [N, Fs]][, ids [N]])``, the last two shared by the batch (the tables themselves).

    ``w.batch(i, out=buffers)`` fills caller-owned buffers in place: ``buffers`` is a tuple laid out like the batch
    tuple whose entries are tensors of the batch's shapes and dtypes, or None for a piece to allocate.  On the ``hip``
    backend a batch is one launch per part it touches and never synchronises.  ``w._last_backend`` records which
    backend formed the last batch."""

    def __init__(self, wide_values, input_len: int, pred_len: int, mode: str = "direct",
                 recursive_pred_len: Optional[int] = None, stride: int = 1, valid_mask=None, series_static=None,
                 series_ids=None, time_features=None, batch_size: int = 256, layout: str = "series", device=None,
                 backend: Optional[str] = None) -> None:
        part = _Part(wide_values, input_len, pred_len, mode, recursive_pred_len, stride, valid_mask, series_static,
                     series_ids, time_features, device)
        self._setup([part], batch_size, layout, backend)

    def _setup(self, parts: List[_Part], batch_size, layout, backend) -> None:
        if layout not in LAYOUTS:
            raise ValueError(f"layout {layout!r} is not 'series' or 'wide'")
        if backend not in (None, "hip", "torch"):
            raise ValueError(f"backend {backend!r} is not 'hip', 'torch' or None")
        if int(batch_size) < 1:
            raise ValueError(f"batch_size={batch_size} is not positive")
        self._parts = parts
        self.layout, self.batch_size = layout, int(batch_size)
        self.device = parts[0].device
        on_gpu = self.device.type == "cuda"
        if backend == "hip" and not on_gpu:
            raise ValueError("backend 'hip' takes tables on a ROCm device")
        self.backend = backend if backend is not None else (DEFAULT_BACKEND[layout] if on_gpu else "torch")
        self._last_backend: Optional[str] = None
        self._bounds = np.concatenate([[0], np.cumsum([p.items(layout) for p in parts], dtype=np.int64)])
        p0 = parts[0]
        self.input_len, self.target_len, self.n_series = p0.L, p0.H, p0.N
        self._F, self._Fs, self._has_static, self._has_ids = p0.F, p0.Fs, p0.statics is not None, p0.ids is not None

    @classmethod
    def concat(cls, windows: Sequence["DeviceWindows"], batch_size: Optional[int] = None,
               backend: Optional[str] = None) -> "DeviceWindows":
        """The items of ``windows[0]``, then ``windows[1]``, ... as ``ConcatDataset`` orders them, batched together: a
        batch that touches two parts is two launches into disjoint row ranges of the same outputs.  The parts must
        agree on the layout, the device, ``L``, ``H``, ``F``, ``Fs`` and on which optional pieces exist (the
        reference's collate would fail mid-epoch); wide parts also on ``N``, and they carry no statics or ids."""
        ws = list(windows)
        if not ws or not all(isinstance(w, DeviceWindows) for w in ws):
            raise ValueError("concat takes a non-empty sequence of DeviceWindows")
        parts = [p for w in ws for p in w._parts]
        first = ws[0]
        for w in ws[1:]:
            if w.layout != first.layout or w.device != first.device:
                raise ValueError(f"concat: layouts / devices differ: {first.layout} on {first.device} and {w.layout} on "
                                 f"{w.device}")
        names = ("input_len", "target length", "time features F", "series_static given", "static features Fs",
                 "series_ids given")
        for p in parts[1:]:
            for name, a, b in zip(names, parts[0].signature(), p.signature()):
                if a != b:
                    raise ValueError(f"concat: parts disagree on {name}: {a} and {b}")
        if first.layout == "wide":
            if any(p.N != parts[0].N for p in parts):
                raise ValueError("concat: wide parts disagree on the number of series")
            if len(parts) > 1 and (parts[0].statics is not None or parts[0].ids is not None):
                raise ValueError("concat: wide parts share their statics and ids with the batch; concatenate tables "
                                 "without them")
        new = cls.__new__(cls)
        new._setup(parts, first.batch_size if batch_size is None else batch_size, first.layout,
                   backend if backend is not None else first.backend)
        return new

    # ------------------------------------------------------------------ sizes
    @property
    def n_items(self) -> int:
        return int(self._bounds[-1])

    @property
    def n_windows(self) -> int:
        return sum(p.W for p in self._parts)

    @property
    def starts(self) -> np.ndarray:
        """The window start rows (int64), part after part."""
        return np.concatenate([p.starts_host for p in self._parts]).astype(np.int64)

    def __len__(self) -> int:
        return -(-self.n_items // self.batch_size)

    def __iter__(self):
        for i in range(len(self)):
            yield self.batch(i)

    # ------------------------------------------------------------------ batches
    def _shapes(self, B: int):
        L, H, F = self.input_len, self.target_len, self._F
        n = 1 if self.layout == "series" else self.n_series
        marks = ((B, L, F), (B, H, F)) if F else ((B, 0), (B, 0))
        return [(B, L, n), (B, H, n), (B, H, n), *marks]

    def batch(self, i: int, out=None):
        """The ``i``-th batch tuple (see the class); ``out``: a tuple of buffers to fill in place, laid out like the
        batch tuple, None where a piece is to be allocated."""
        nb = len(self)
        i = int(i)
        if not -nb <= i < nb:
            raise IndexError(f"batch {i} of {nb}")
        i %= nb
        k0 = i * self.batch_size
        k1 = min(k0 + self.batch_size, self.n_items)
        B = k1 - k0
        series = self.layout == "series"
        names = ["x", "y", "mask", "x_mark", "y_mark"]
        shapes = self._shapes(B)
        if series and self._has_static:
            names.append("static")
            shapes.append((B, 1, self._Fs))
        if series and self._has_ids:
            names.append("id")
            shapes.append((B, 1))
        n_shared = 0 if series else int(self._has_static) + int(self._has_ids)
        if out is not None and len(out) != len(names) + n_shared:
            raise ValueError(f"batch: out has {len(out)} entries, the batch tuple has {len(names) + n_shared}")
        touched = [(p, max(k0, int(a)) - int(a), min(k1, int(b)) - int(a), max(k0, int(a)) - k0)
                   for p, a, b in zip(self._parts, self._bounds[:-1], self._bounds[1:]) if k0 < b and a < k1]
        if self.backend == "torch" and out is None and len(touched) == 1:
            p, a, b, _ = touched[0]
            res = self._torch_pieces(p, a, b - a)
        else:
            res = []
            for at, (name, shape) in enumerate(zip(names, shapes)):
                dtype = torch.int64 if name == "id" else torch.float32
                buf = None if out is None else out[at]
                if buf is None:
                    buf = torch.empty(shape, dtype=dtype, device=self.device)
                elif (not isinstance(buf, torch.Tensor) or tuple(buf.shape) != shape or buf.dtype != dtype
                      or buf.device != self.device or not buf.is_contiguous()):
                    raise ValueError(f"batch: out[{at}] ({name}) must be a contiguous {dtype} tensor {shape} on "
                                     f"{self.device}, got {tuple(getattr(buf, 'shape', ()))}")
                res.append(buf)
            for p, a, b, r0 in touched:
                rows = {n: t[r0:r0 + b - a] for n, t in zip(names, res) if t.numel()}
                if self.backend == "hip":
                    from . import runtime as rt

                    rt.window_batch(p.X, p.starts, p.starts_host, p.L, p.H, a, b - a, rows, M=p.M, marks=p.marks,
                                    statics=p.statics if "static" in rows else None,
                                    ids=p.ids if "id" in rows else None, layout=self.layout)
                else:
                    for t, src in zip(res, self._torch_pieces(p, a, b - a)):
                        if t.numel():
                            t[r0:r0 + b - a].copy_(src)
        self._last_backend = self.backend
        if not series:
            p = self._parts[0]
            res = list(res) + [t for t in (p.statics, p.ids) if t is not None]
        return tuple(res)

    def _torch_pieces(self, p: _Part, item0: int, count: int) -> list:
        """Items ``item0 .. item0 + count - 1`` of one part as a composition of torch ops on the table's device: the
        pieces in batch-tuple order (without the shared statics and ids of the wide layout)."""
        dev = p.device
        k = torch.arange(item0, item0 + count, device=dev)
        series = self.layout == "series"
        w = torch.div(k, p.N, rounding_mode="floor") if series else k
        s = p.starts[w].to(torch.int64)
        rx = s[:, None] + torch.arange(p.L, device=dev)[None, :]                 # [B, L] table rows of x
        ry = (s + p.L)[:, None] + torch.arange(p.H, device=dev)[None, :]         # [B, H] table rows of y
        if series:
            col = (k - w * p.N)[:, None]
            x, y = p.X[rx, col].unsqueeze(-1), p.X[ry, col].unsqueeze(-1)
            mask = p.M[ry, col].unsqueeze(-1) if p.M is not None else torch.ones_like(y)
        else:
            x, y = p.X[rx], p.X[ry]
            mask = p.M[ry] if p.M is not None else torch.ones_like(y)
        if p.marks is not None:
            xm, ym = p.marks[rx], p.marks[ry]
        else:
            xm = torch.empty(count, 0, dtype=torch.float32, device=dev)
            ym = torch.empty(count, 0, dtype=torch.float32, device=dev)
        res = [x, y, mask, xm, ym]
        if series and p.statics is not None:
            res.append(p.statics[col[:, 0]].unsqueeze(1))
        if series and p.ids is not None:
            res.append(p.ids[col[:, 0]].unsqueeze(1))
        return res
