"""Sliding windows formed on the device: the batches of a rolling-origin backtest without a host loader.

``DeviceWindows`` holds the wide table ``[T, N]`` (values, validity mask, time features, statics, ids) on the device
once and forms every batch that the reference's ``SlidingWindowDataset`` (data/dataset.py:29-204) behind a
``DataLoader(shuffle=False, drop_last=False)`` would yield - the same item order, shapes, dtypes and bits - with one
``ftn_window_batch`` launch (csrc/windows.hip) and no host synchronisation, so
``score.eval_metrics(model, DeviceWindows(...), ...)`` is a whole backtest whose only synchronisation is the scorer's
``result()``.

With ``shuffle``, ``drop_last``, ``seed`` or ``augment`` it is the training loader, ``DataLoader(..., shuffle=True,
drop_last=True, augment={"add_noise_std", "time_shift"})`` (train.py:933, data/dataset.py:181-193): an epoch's order,
every item's time shift and every element's noise are pure functions of ``(seed, epoch)`` on the project's own
Philox4x32-10 (``nbdist.philox4x32``; the definitions are in include/flowtimes.h, "training windows"), formed by one
``ftn_window_gather`` launch per part (csrc/windows_gather.hip) from series-major copies of the tables.  The
reference draws from numpy's and torch's global state; those draws cannot be restated, these can (DESIGN.md section
8).  Calendar-feature construction from a time index and weighted or stratified sampling are not part of it
(``gather`` takes any item list).

``layout="series"`` is the reference's: an item is one series of one window, item ``k`` = window ``k // N``, series
``k % N``.  ``layout="wide"`` is this project's ``[B, L, N]`` layout: an item is one window with all its series.

Backends: ``hip`` for fp32 tables on a ROCm device, a ``torch`` composition (index arithmetic and advanced indexing,
no Python loop over items) anywhere; both give the same bits for the order, the shift and every copy (the noise of
the ``torch`` backend is evaluated with numpy's fp64 ``log``, ``cos`` and ``sin`` on the host and may differ from
the kernel's in the last fp32 place).
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch

LAYOUTS = ("series", "wide")
# The backend ``backend=None`` takes for a ROCm table, per layout (DESIGN.md section 4 "Device windows": HIP is the
# default of a layout only where it was at or below the torch composition at every measured shape of that layout).
DEFAULT_BACKEND = {"series": "hip", "wide": "hip"}
# The same rule for the shuffled or augmented batches of the training loader (DESIGN.md section 4 "Training windows").
DEFAULT_TRAIN_BACKEND = {"series": "hip", "wide": "hip"}
AUGMENT_KEYS = ("add_noise_std", "time_shift")
_M32 = 0xFFFFFFFF


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

        self._series_major = None

    def series_major(self):
        """``(XT, MT)``: the series-major copies ``[N, T]`` of the values and the validity (None without one) that
        ``ftn_window_gather`` reads in the series layout, made once on first use: a snapshot of the tables as they
        were then (``DeviceWindows.refresh`` drops it)."""
        if self._series_major is None:
            self._series_major = (self.X.t().contiguous(), None if self.M is None else self.M.t().contiguous())
        return self._series_major

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
    backend formed the last batch.

    The training loader: any of ``shuffle=True``, ``drop_last=True``, ``seed`` and ``augment={"add_noise_std": sd,
    "time_shift": ts}`` (the reference's dict; both keys optional).  With all four at their defaults nothing above
    changes.  Otherwise the batches are those of epoch ``w.epoch`` (``w.set_epoch(e)``; ``0 <= e < 2^30``):
    ``iter(w)`` yields the current epoch's batches and advances ``w.epoch`` when the iterator is created, so every
    pass of ``fit.refit_heads(model, w, epochs=n)`` is another epoch; ``w.order(epoch=None)`` is the epoch's item
    order on the device, ``w.batch(i, out=None, epoch=None)`` its ``i``-th batch - positions ``i B ..`` of the order,
    ``len(w)`` honouring ``drop_last`` - and ``w.gather(items, out=None, epoch=None)`` the batch of an explicit item
    list.  One time shift moves ``x``, ``y``, ``mask`` and both marks of an item together; the noise touches ``x``
    only.  On the ``hip`` backend a batch is one ``ftn_window_gather`` launch per part and never synchronises; the
    series layout reads series-major copies of the tables made once on first use - a snapshot: after changing a
    table in place, ``w.refresh()`` drops it."""

    def __init__(self, wide_values, input_len: int, pred_len: int, mode: str = "direct",
                 recursive_pred_len: Optional[int] = None, stride: int = 1, valid_mask=None, series_static=None,
                 series_ids=None, time_features=None, batch_size: int = 256, layout: str = "series", device=None,
                 backend: Optional[str] = None, shuffle: bool = False, drop_last: bool = False, seed: int = 0,
                 augment: Optional[dict] = None) -> None:
        train = self._train_args(shuffle, drop_last, seed, augment)     # argument errors before any work
        part = _Part(wide_values, input_len, pred_len, mode, recursive_pred_len, stride, valid_mask, series_static,
                     series_ids, time_features, device)
        self._setup([part], batch_size, layout, backend, train)

    @staticmethod
    def _train_args(shuffle, drop_last, seed, augment):
        """``(default, shuffle, drop_last, seed, time_shift, add_noise_std)``, validated; ``default``: all four
        arguments are at their defaults and the loader is the validation loader."""
        aug = {} if augment is None else dict(augment)
        unknown = sorted(set(aug) - set(AUGMENT_KEYS))
        if unknown:
            raise ValueError(f"augment: unknown keys {unknown}; the keys are {AUGMENT_KEYS}")
        from .runtime import window_epoch_check

        seed, _, ts, sd = window_epoch_check("DeviceWindows", seed, 0, aug.get("time_shift", 0) or 0,
                                             aug.get("add_noise_std", 0.0) or 0.0)
        default = not shuffle and not drop_last and seed == 0 and augment is None
        return default, bool(shuffle), bool(drop_last), seed, ts, sd

    def _setup(self, parts: List[_Part], batch_size, layout, backend, train=None) -> None:
        self._default, self.shuffle, self.drop_last, self.seed, self.time_shift, self.add_noise_std = (
            train if train is not None else self._train_args(False, False, 0, None))
        self.epoch = 0
        self._orders: dict = {}
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
        table = DEFAULT_BACKEND if self._default else DEFAULT_TRAIN_BACKEND
        self.backend = backend if backend is not None else (table[layout] if on_gpu else "torch")
        self._last_backend: Optional[str] = None
        self._bounds = np.concatenate([[0], np.cumsum([p.items(layout) for p in parts], dtype=np.int64)])
        p0 = parts[0]
        self.input_len, self.target_len, self.n_series = p0.L, p0.H, p0.N
        self._F, self._Fs, self._has_static, self._has_ids = p0.F, p0.Fs, p0.statics is not None, p0.ids is not None

    @classmethod
    def concat(cls, windows: Sequence["DeviceWindows"], batch_size: Optional[int] = None,
               backend: Optional[str] = None, shuffle: Optional[bool] = None, drop_last: Optional[bool] = None,
               seed: Optional[int] = None, augment: Optional[dict] = None) -> "DeviceWindows":
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
        if shuffle is None and drop_last is None and seed is None and augment is None and first._default:
            train = None
        else:                                                   # the first loader's, each overridden where given
            train = cls._train_args(first.shuffle if shuffle is None else shuffle,
                                    first.drop_last if drop_last is None else drop_last,
                                    first.seed if seed is None else seed,
                                    augment if augment is not None else
                                    {"add_noise_std": first.add_noise_std, "time_shift": first.time_shift})
        new = cls.__new__(cls)
        new._setup(parts, first.batch_size if batch_size is None else batch_size, first.layout,
                   backend if backend is not None else first.backend, train)
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
        if self.drop_last:
            return self.n_items // self.batch_size
        return -(-self.n_items // self.batch_size)

    def __iter__(self):
        if self._default:
            return (self.batch(i) for i in range(len(self)))
        epoch = self._epoch_arg(None)                           # taken now: the iterator keeps its epoch
        self.epoch += 1
        return (self.batch(i, epoch=epoch) for i in range(len(self)))

    def refresh(self) -> None:
        """Drops the series-major copies, so that the next batch makes them anew.  Every other path reads the tables
        in place; the copies are a snapshot taken at the first training batch of the series layout on the ``hip``
        backend, so call this after changing a table in place (a scaler's transform into the same tensor, say)."""
        for p in self._parts:
            p._series_major = None

    # ------------------------------------------------------------------ epochs
    def set_epoch(self, epoch: int) -> None:
        """The epoch the next ``iter(w)`` (and ``batch`` / ``gather`` / ``order`` without ``epoch=``) takes."""
        self.epoch = self._epoch_arg(epoch)

    def _epoch_arg(self, epoch) -> int:
        from .runtime import window_epoch_check

        return window_epoch_check("DeviceWindows", 0, self.epoch if epoch is None else epoch)[1]

    def _key(self):
        return self.seed & _M32, self.seed >> 32

    def order(self, epoch: Optional[int] = None) -> torch.Tensor:
        """The epoch's order: int64 ``[n_items]`` on the device, position ``p`` of the epoch is item ``order[p]`` -
        the stable ascending argsort of ``key64`` with ``shuffle``, else the identity.  Cached per epoch (the two
        most recent)."""
        epoch = self._epoch_arg(epoch)
        if epoch in self._orders:
            return self._orders[epoch]
        n = self.n_items
        if not self.shuffle or n == 0:
            order = torch.arange(n, dtype=torch.int64, device=self.device)
        else:
            if self.backend == "hip":
                from . import runtime as rt

                keys = rt.epoch_keys(n, self.seed, epoch, self.device)
            else:
                from .nbdist import philox4x32

                k = torch.arange(n, dtype=torch.int64, device=self.device)
                x, y, _, _ = philox4x32((k & _M32, k >> 32, 0, epoch << 2), self._key())
                keys = (x - ((x >> 31) << 32)) * (1 << 32) + y  # the signed int64 with bits (x << 32) | y
            order = torch.argsort(keys, stable=True)
        while len(self._orders) >= 2:
            self._orders.pop(next(iter(self._orders)))
        self._orders[epoch] = order
        return order

    # ------------------------------------------------------------------ batches
    def _shapes(self, B: int):
        L, H, F = self.input_len, self.target_len, self._F
        n = 1 if self.layout == "series" else self.n_series
        marks = ((B, L, F), (B, H, F)) if F else ((B, 0), (B, 0))
        return [(B, L, n), (B, H, n), (B, H, n), *marks]

    def _pieces(self, B: int, out, who: str):
        """The names and shapes of a batch of ``B`` items, after checking the length of ``out``."""
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
            raise ValueError(f"{who}: out has {len(out)} entries, the batch tuple has {len(names) + n_shared}")
        return names, shapes

    def _buffers(self, names, shapes, out, who: str) -> list:
        """The output tensors of a batch: the caller's where given (checked), else new ones."""
        res = []
        for at, (name, shape) in enumerate(zip(names, shapes)):
            dtype = torch.int64 if name == "id" else torch.float32
            buf = None if out is None else out[at]
            if buf is None:
                buf = torch.empty(shape, dtype=dtype, device=self.device)
            elif (not isinstance(buf, torch.Tensor) or tuple(buf.shape) != shape or buf.dtype != dtype
                  or buf.device != self.device or not buf.is_contiguous()):
                raise ValueError(f"{who}: out[{at}] ({name}) must be a contiguous {dtype} tensor {shape} on "
                                 f"{self.device}, got {tuple(getattr(buf, 'shape', ()))}")
            res.append(buf)
        return res

    def gather(self, items, out=None, epoch: Optional[int] = None):
        """The batch tuple of the explicit ``items`` (global item indices; an int64 tensor or a sequence), item
        ``items[r]`` in row ``r``, with the time shift and the noise of ``epoch`` (default: the current one) - a pure
        function of ``(seed, epoch, item)``, whatever batch and row an item lands in.  Host items are range-checked;
        a device tensor is not read back: a row whose item is out of range keeps what the ``out=`` buffer held, and
        is undefined (uninitialised memory) in a piece that was allocated here."""
        epoch = self._epoch_arg(epoch)
        if isinstance(items, torch.Tensor) and items.device.type != "cpu":
            if items.dim() != 1 or items.dtype != torch.int64 or items.device != self.device:
                raise ValueError(f"gather: device items must be an int64 vector on {self.device}")
            items = items.contiguous()
        else:
            host = np.asarray(items.numpy() if isinstance(items, torch.Tensor) else items)
            if host.ndim != 1 or host.dtype.kind not in "iu":
                raise ValueError("gather: items must be a vector of integers")
            if host.size and (int(host.min()) < 0 or int(host.max()) >= self.n_items):
                raise ValueError(f"gather: items must be in 0..{self.n_items - 1}, got {int(host.min())}.."
                                 f"{int(host.max())}")
            items = torch.from_numpy(np.ascontiguousarray(host.astype(np.int64))).to(self.device)
        B = int(items.numel())
        if B < 1:
            raise ValueError("gather: no items")
        names, shapes = self._pieces(B, out, "gather")
        res = self._buffers(names, shapes, out, "gather")
        for p, a in zip(self._parts, self._bounds[:-1]):
            if p.items(self.layout) == 0:
                continue
            rows = {n: t for n, t in zip(names, res) if t.numel()}
            if self.backend == "hip":
                from . import runtime as rt

                XT, MT = p.series_major() if self.layout == "series" else (None, None)
                rt.window_gather(p.X, p.starts, p.starts_host, p.L, p.H, int(a), items, rows, XT=XT, M=p.M, MT=MT,
                                 marks=p.marks, statics=p.statics if "static" in rows else None,
                                 ids=p.ids if "id" in rows else None, layout=self.layout,
                                 time_shift=self.time_shift, noise_std=self.add_noise_std, seed=self.seed, epoch=epoch)
            else:
                self._torch_gather(p, int(a), items, rows, epoch)
        self._last_backend = self.backend
        if self.layout != "series":
            p = self._parts[0]
            res = list(res) + [t for t in (p.statics, p.ids) if t is not None]
        return tuple(res)

    def _torch_gather(self, p: _Part, item_lo: int, items: torch.Tensor, rows: dict, epoch: int) -> None:
        """The definition of ``ftn_window_gather`` as torch ops (the noise through numpy's fp64 on the host): the rows
        of ``rows`` whose item belongs to part ``p`` are written, the others keep their content."""
        from .nbdist import _mulhilo32, philox4x32

        n = p.items(self.layout)
        if n == 0:
            return
        valid = (items >= item_lo) & (items < item_lo + n)
        kl = (items - item_lo).clamp(0, n - 1)
        start = None
        if self.time_shift:
            k = item_lo + kl                                    # the generator counts global items
            x = philox4x32((k & _M32, k >> 32, 0, (epoch << 2) | 1), self._key())[0]
            w = torch.div(kl, p.N, rounding_mode="floor") if self.layout == "series" else kl
            delta = _mulhilo32(2 * self.time_shift + 1, x)[0] - self.time_shift
            start = (p.starts[w].to(torch.int64) + delta).clamp(0, p.T - p.L - p.H)
        pieces = self._torch_pieces(p, kl, None, start=start)
        if self.add_noise_std > 0:
            pieces[0] = self._torch_noise(pieces[0], item_lo + kl, epoch)
        names = ["x", "y", "mask", "x_mark", "y_mark"]          # the order of _torch_pieces
        if self.layout == "series":
            names += [n_ for n_, t in (("static", p.statics), ("id", p.ids)) if t is not None]
        for name, src in zip(names, pieces):
            dst = rows.get(name)
            if dst is not None:
                sel = valid.reshape((-1,) + (1,) * (dst.dim() - 1))
                dst.copy_(torch.where(sel, src.reshape(dst.shape), dst))

    def _torch_noise(self, x: torch.Tensor, k: torch.Tensor, epoch: int) -> torch.Tensor:
        """``fl32(double(x) + add_noise_std z)`` with the Box-Muller pairs of the definition, in numpy's fp64."""
        from .nbdist import philox4x32

        B = x.shape[0]
        J = x.numel() // B
        q = torch.arange((J + 3) // 4, dtype=torch.int64, device=k.device)
        words = philox4x32(((k & _M32)[:, None], (k >> 32)[:, None], q[None, :], (epoch << 2) | 2), self._key())
        a, b, c, d = ((w.expand(B, q.numel()).cpu().numpy().astype(np.float64) + 0.5) * 2.0 ** -32 for w in words)
        z = np.empty((B, q.numel(), 4), dtype=np.float64)
        for lane, (u1, u2) in ((0, (a, b)), (2, (c, d))):
            r = np.sqrt(-2.0 * np.log(u1))
            z[:, :, lane] = r * np.cos(2 * np.pi * u2)
            z[:, :, lane + 1] = r * np.sin(2 * np.pi * u2)
        z = z.reshape(B, -1)[:, :J]
        xh = x.detach().cpu().numpy().reshape(B, J).astype(np.float64)
        out = (xh + np.float64(self.add_noise_std) * z).astype(np.float32)
        return torch.from_numpy(out).to(x.device).reshape(x.shape)

    def batch(self, i: int, out=None, epoch: Optional[int] = None):
        """The ``i``-th batch tuple (see the class); ``out``: a tuple of buffers to fill in place, laid out like the
        batch tuple, None where a piece is to be allocated.  For a training loader the batch is that of ``epoch``
        (default: the current one): a pure function of ``(seed, epoch, i)``."""
        nb = len(self)
        i = int(i)
        if not -nb <= i < nb:
            raise IndexError(f"batch {i} of {nb}")
        i %= nb
        k0 = i * self.batch_size
        k1 = min(k0 + self.batch_size, self.n_items)
        B = k1 - k0
        if not self._default:
            epoch = self._epoch_arg(epoch)
            self._pieces(B, out, "batch")                       # a wrong out fails before the order is formed
            return self.gather(self.order(epoch)[k0:k1], out=out, epoch=epoch)
        series = self.layout == "series"
        names, shapes = self._pieces(B, out, "batch")
        touched = [(p, max(k0, int(a)) - int(a), min(k1, int(b)) - int(a), max(k0, int(a)) - k0)
                   for p, a, b in zip(self._parts, self._bounds[:-1], self._bounds[1:]) if k0 < b and a < k1]
        if self.backend == "torch" and out is None and len(touched) == 1:
            p, a, b, _ = touched[0]
            res = self._torch_pieces(p, a, b - a)
        else:
            res = self._buffers(names, shapes, out, "batch")
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

    def _torch_pieces(self, p: _Part, item0, count, start: Optional[torch.Tensor] = None) -> list:
        """Items ``item0 .. item0 + count - 1`` of one part - or the items of the int64 tensor ``item0`` - as a
        composition of torch ops on the table's device: the pieces in batch-tuple order (without the shared statics
        and ids of the wide layout).  ``start``: the items' start rows where they are not the windows' own."""
        dev = p.device
        if isinstance(item0, torch.Tensor):
            k, count = item0, int(item0.numel())
        else:
            k = torch.arange(item0, item0 + count, device=dev)
        series = self.layout == "series"
        w = torch.div(k, p.N, rounding_mode="floor") if series else k
        s = p.starts[w].to(torch.int64) if start is None else start
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
