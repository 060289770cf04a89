"""Shared by the device-window tests: the fixture of tests/golden/windows_cases.npz (the reference's loader batches),
builders of ``DeviceWindows`` from it, an item-by-item numpy restatement of both layouts, the form rule of
``ftn_window_batch_form`` restated from the header, and the shape sweep the forms table and the GPU tests walk."""
import json
from pathlib import Path

import numpy as np
import torch

GOLDEN = Path(__file__).resolve().parent / "golden" / "windows_cases.npz"
PIECES = ("x", "y", "mask", "x_mark", "y_mark", "static", "id")
TILE = (64, 32)


def fixture():
    """``(meta, arrays)``: the case table and every array of the npz."""
    with np.load(GOLDEN) as z:
        arrays = {k: z[k] for k in z.files if k != "cases"}
        meta = json.loads(str(z["cases"]))
    return meta, arrays


def part_tables(arrays, case, k):
    return {n: arrays.get(f"{case}:p{k}:{n}") for n in ("X", "M", "marks", "static", "ids")}


def build(ftn, meta, arrays, case, device="cpu", backend=None, layout="series", batch_size=None):
    """The ``DeviceWindows`` of a fixture case (a ``concat`` when it has several parts)."""
    DW = ftn.windows.DeviceWindows
    m = meta[case]
    bs = m["batch"] if batch_size is None else batch_size
    ws = []
    for k, p in enumerate(m["parts"]):
        t = part_tables(arrays, case, k)
        ws.append(DW(t["X"], p["L"], p["pred_len"], p["mode"], recursive_pred_len=p["recursive_pred_len"],
                     stride=p["stride"], valid_mask=t["M"], series_static=t["static"], series_ids=t["ids"],
                     time_features=t["marks"], batch_size=bs, layout=layout, device=device, backend=backend))
    return ws[0] if len(ws) == 1 else DW.concat(ws, batch_size=bs)


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Shape, dtype and every bit (NaN payloads and the sign of zero included)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return bool(torch.equal(a.cpu(), b.cpu()))


def batches_same(got, want) -> bool:
    return len(got) == len(want) and all(same_bits(torch.as_tensor(g), torch.as_tensor(w)) for g, w in zip(got, want))


def items_numpy(X, M, marks, static, ids, L, H, stride, layout, k0, k1):
    """Items k0 .. k1 - 1 by the definition, one item at a time: the batch tuple as numpy arrays."""
    T, N = X.shape
    starts = np.arange(0, T - L - H + 1, max(1, stride)) if T >= L + H else np.zeros(0, np.int64)
    F = 0 if marks is None else marks.shape[1]
    rows = {n: [] for n in PIECES}
    for k in range(k0, k1):
        w, i = (k // N, k % N) if layout == "series" else (k, slice(None))
        s = int(starts[w])
        e = s + L
        cut = (lambda a, lo, hi: a[lo:hi, i:i + 1]) if layout == "series" else (lambda a, lo, hi: a[lo:hi, :])
        rows["x"].append(cut(X, s, e))
        rows["y"].append(cut(X, e, e + H))
        rows["mask"].append(cut(M, e, e + H) if M is not None else np.ones_like(cut(X, e, e + H)))
        rows["x_mark"].append(marks[s:e] if F else np.zeros(0, np.float32))
        rows["y_mark"].append(marks[e:e + H] if F else np.zeros(0, np.float32))
        if layout == "series" and static is not None:
            rows["static"].append(static[i:i + 1])
        if layout == "series" and ids is not None:
            rows["id"].append(ids[i:i + 1])
    out = [np.stack(rows[n]) for n in PIECES if rows[n]]
    if layout == "wide":
        out += [t for t in (static, ids) if t is not None]
    return out


def want_form(layout, N, L, H, F=0, outs=("x", "y", "mask"), x_stride=None, m_stride=None, marks_stride=None,
              has_mask=True, misalign=None):
    """The form rule of include/flowtimes.h, restated: a piece moves 16 bytes a lane when its columns (the series; the
    marks' features), its row strides and - for the transposed pieces of the series layout - its time steps are
    multiples of 4 and its table and output are on the 16-byte grid."""
    mis = misalign or {}
    xs = N if x_stride is None else x_stride
    ms = N if m_stride is None else m_stride
    ks = F if marks_stride is None else marks_stride
    src = {"x": ("X", xs, N, L), "y": ("X", xs, N, H), "mask": ("M" if has_mask else None, ms, N, H),
           "x_mark": ("marks", ks, F, 4), "y_mark": ("marks", ks, F, 4)}
    vec = []
    for name in PIECES[:5]:
        if name not in outs:
            continue
        tab, stride, cols, steps = src[name]
        ok = cols % 4 == 0 and (tab is None or (stride % 4 == 0 and mis.get(tab, 0) % 16 == 0))
        if layout == "series" and name in ("x", "y", "mask"):
            ok = ok and steps % 4 == 0
        if ok and mis.get(name, 0) % 16 == 0:
            vec.append(name)
    tiled = layout == "series" and any(n in outs for n in ("x", "y", "mask"))
    return {"vec": tuple(vec), "tile": TILE if tiled else None}


# ---- the sweep: every N x L of the issue, the other parameters rotating through their values ----
SWEEP_N = (1, 5, 63, 64, 65, 193)
SWEEP_L = (1, 7, 28, 63, 64, 65, 130)
SWEEP_H = (1, 3, 7)
SWEEP_STRIDE = (1, 2, 5, None)                                   # None: larger than T, one window
SWEEP_F = (0, 1, 3, 5)
SWEEP_FS = (0, 2)


def sweep(N):
    """The shapes swept at ``N`` series: one per L, with H, stride, F, Fs, ids and mask rotating so that every value
    of each meets every N; plus L = 28 and 64 with H = 4 and F = 4, where every piece can take the 16-byte form."""
    at = SWEEP_N.index(N)
    out = []
    for j, L in enumerate(SWEEP_L):
        r = at + j
        H = SWEEP_H[r % 3]
        stride = SWEEP_STRIDE[r % 4]
        windows = 1 if stride is None else 3
        T = L + H + (0 if stride is None else stride * (windows - 1) + (r % 2))
        out.append(dict(N=N, L=L, H=H, T=T, stride=T + 1 if stride is None else stride, F=SWEEP_F[(r // 2) % 4],
                        Fs=SWEEP_FS[r % 2], ids=r % 3 != 1, mask=r % 4 != 2))
    for L in (28, 64):
        out.append(dict(N=N, L=L, H=4, T=L + 4 + 4, stride=2, F=4, Fs=2, ids=True, mask=True))
    return out


def sweep_tables(shape, seed):
    """Seeded tables of a sweep shape with -0, inf, and NaNs of distinct payloads among the values."""
    g = np.random.default_rng(seed)
    T, N, F, Fs = shape["T"], shape["N"], shape["F"], shape["Fs"]
    X = g.standard_normal((T, N)).astype(np.float32)
    flat = X.reshape(-1).view(np.uint32)
    special = np.array([0x80000000, 0x7f800000, 0xff800000, 0x7fc00001, 0xffc12345, 0x7f800001, 0x00000001], np.uint32)
    pos = g.permutation(flat.size)[:min(flat.size, special.size)]
    flat[pos] = special[:pos.size]
    t = {"X": X, "M": None, "marks": None, "static": None, "ids": None}
    if shape["mask"]:
        t["M"] = (g.random((T, N)) >= 0.3).astype(np.float32)
    if F:
        t["marks"] = g.standard_normal((T, F)).astype(np.float32)
    if Fs:
        t["static"] = g.standard_normal((N, Fs)).astype(np.float32)
    if shape["ids"]:
        t["ids"] = (g.permutation(4 * N)[:N].astype(np.int64) << 33) + 7       # both words of an id carry bits
    return t


def batch_sizes(N, n_items):
    """1, N - 1, N, N + 1, 2 N + 3 and one batch that spans every window."""
    return sorted({b for b in (1, N - 1, N, N + 1, 2 * N + 3, n_items) if b >= 1})
