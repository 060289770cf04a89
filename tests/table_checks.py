"""Shared by the table-preparation tests: the fixture of tests/golden/table_cases.npz (the reference's outputs), an
fp64 restatement of the features and the scaler pairs with the rounding points of include/flowtimes.h, the form rules
of ``ftn_table_*_form`` restated from the header, and the shape sweep the forms table and the GPU tests walk."""
import json
from pathlib import Path

import numpy as np
import torch

GOLDEN = Path(__file__).resolve().parent / "golden" / "table_cases.npz"
FITS = [("zscore", True), ("zscore", False), ("minmax", True), ("minmax", False)]
FEATURES = ("mean", "std", "diff_std", "seasonal_strength", "dominant_period")
COLS, BINS, CHUNK, PARTIALS_MAX = 64, 128, 128, 32

# The sweep of the issue, plus the two lengths on either side of the spectrum kernel's staging-chunk boundaries
# (a chunk is CHUNK = 128 rows: 128 | 129 is one chunk against two, 256 | 257 two against three; 127, 129, 255 and 257
# are in the issue's list already).  The bin block of 128 bins ends at T = 257, so 256 .. 258 cross that as well.
SWEEP_T = (1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 63, 64, 65, 66, 127, 129, 255, 257) + (128, 130, 256, 258)
SWEEP_N = (1, 5, 31, 32, 33, 63, 64, 65, 193)
MASKS = ("none", "gaps", "column")
LAYOUTS = ("dense", "slice", "off16", "slice4")
# lengths at which the extra cases run the 16-byte forms on an aligned column slice (row stride > N): the staging-chunk
# and bin-block boundaries and one chunk's two sides of 64
BOUNDARY_T = (64, 65, 127, 128, 129, 130, 255, 256, 257, 258)


def fixture():
    """``(meta, arrays)``: the table descriptions and every array of the npz."""
    with np.load(GOLDEN) as z:
        arrays = {k: z[k] for k in z.files if k != "meta"}
        meta = json.loads(str(z["meta"]))
    return meta, arrays


def fit_key(name, method, per_series):
    return f"{name}:{method}:{'ps' if per_series else 'gl'}"


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return bool(torch.equal(a.cpu(), b.cpu()))


def ulps(got, want) -> np.ndarray:
    """|got - want| in units of the fp32 spacing at ``want`` (0 where both are the same value or both NaN)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    both_nan = np.isnan(got) & np.isnan(want)
    sp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    with np.errstate(invalid="ignore"):
        d = np.abs(got - want) / sp
    return np.where(both_nan | (got == want), 0.0, d)


# ---------------------------------------------------------------- the fp64 restatement
def moments64(X, M=None, clip=False, mean32=None):
    """Count, fp32 mean (sum in fp64, rounded once; ``mean32``: use this one), centred sum of squares of
    fp32(x - mean) in fp64, min and max per column."""
    x = np.asarray(X, np.float32)
    if clip:
        x = np.where(x < 0, np.float32(0), x)
    ok = np.ones(x.shape, bool) if M is None else np.asarray(M) > 0
    cnt = ok.sum(axis=0).astype(np.float64)
    s = np.where(ok, x.astype(np.float64), 0.0).sum(axis=0)
    mean = (s / np.maximum(cnt, 1.0)).astype(np.float32) if mean32 is None else np.asarray(mean32, np.float32)
    d = (x - mean[None, :]).astype(np.float32)
    css = np.where(ok, d.astype(np.float64) ** 2, 0.0).sum(axis=0)
    with np.errstate(invalid="ignore"):
        mn = np.where(ok, x, np.inf).min(axis=0, initial=np.inf)
        mx = np.where(ok, x, -np.inf).max(axis=0, initial=-np.inf)
    return dict(cnt=cnt, sum=s, mean=mean, css=css, min=mn.astype(np.float32), max=mx.astype(np.float32))


def std32(css, cnt):
    """sqrt(fp32(css / max(cnt, 1))): the variance rounded once, the root once."""
    return np.sqrt((css / np.maximum(cnt, 1.0)).astype(np.float32)).astype(np.float32)


def diffs_of(X, M):
    x = np.asarray(X, np.float32)
    dx = (x[1:] - x[:-1]).astype(np.float32)
    ok = np.ones(dx.shape, np.float32) if M is None else ((np.asarray(M)[1:] > 0) & (np.asarray(M)[:-1] > 0)).astype(np.float32)
    return dx, ok


def power64(X, M, mean32):
    """P[f - 1][n] for f = 1 .. T // 2 in fp64 of d = fp32(x - mean) under the mask."""
    x = np.asarray(X, np.float32)
    d = (x - np.asarray(mean32, np.float32)[None, :]).astype(np.float32)
    if M is not None:
        d = np.where(np.asarray(M) > 0, d, np.float32(0))
    return np.abs(np.fft.rfft(d.astype(np.float64), axis=0))[1:] ** 2


def features64(X, M=None, mean32=None, dmean32=None):
    """``(features [N, 5] fp32, P64 [T // 2, N])`` by the definition of include/flowtimes.h in fp64."""
    T, N = np.shape(X)
    m = moments64(X, M, mean32=mean32)
    out = np.zeros((N, 5), np.float32)
    out[:, 0], out[:, 1] = m["mean"], std32(m["css"], m["cnt"])
    P = np.zeros((0, N))
    if T > 1:
        dx, ok = diffs_of(X, M)
        dm = moments64(dx, ok, mean32=dmean32)
        out[:, 2] = std32(dm["css"], dm["cnt"])
        P = power64(X, M, m["mean"])
        tot = P.sum(axis=0)
        peak = P.max(axis=0)
        f = P.argmax(axis=0) + 1
        out[:, 3] = (peak.astype(np.float32) / np.maximum(tot.astype(np.float32), np.float32(1e-6))).astype(np.float32)
        out[:, 4] = np.where(tot.astype(np.float32) > np.float32(1e-6), (float(T) / f).astype(np.float32), 0.0)
    return out, P


def pairs64(X, method, per_series, eps=1e-8, clip=False):
    """The scaler pairs [N, 2] by the definition in fp64 (moments as above, then the reference's eps rule)."""
    x = np.asarray(X, np.float32)
    if clip:
        x = np.where(x < 0, np.float32(0), x)
    N = x.shape[1]
    if not per_series:
        x = x.reshape(-1, 1)
    m = moments64(x)
    if method == "zscore":
        if per_series:
            sd = std32(m["css"], m["cnt"])
            sd = np.where(sd < np.float32(eps), np.float32(1), sd)
        else:                                                   # centred around the fp32 global mean, in fp64 throughout
            css = ((x.astype(np.float64) - np.float64(m["mean"][0])) ** 2).sum(axis=0)
            sd = std32(css, m["cnt"])
            sd = np.where(sd.astype(np.float64) >= eps, sd, np.float32(1))
        pr = np.stack([m["mean"], sd], axis=1).astype(np.float64)
    else:
        pr = np.stack([m["min"], m["max"]], axis=1).astype(np.float64)
    return pr if per_series else np.repeat(pr, N, axis=0)


# ---------------------------------------------------------------- forms, restated from the header
def row_block(T):
    rb = 32
    while -(-T // rb) > PARTIALS_MAX:
        rb *= 2
    return rb


def _vec(N, strides, misalign):
    return N % 4 == 0 and all(s % 4 == 0 for s in strides) and all(m % 16 == 0 for m in misalign)


def want_moments_form(T, N, x_stride=None, m_stride=None, mask=False, misalign=None):
    mis = misalign or {}
    xs, ms = N if x_stride is None else x_stride, N if m_stride is None else m_stride
    vec = _vec(N, [xs] + ([ms] if mask else []), [mis.get("X", 0)] + ([mis.get("M", 0)] if mask else []))
    rb = row_block(T)
    return dict(load_bytes=16 if vec else 4, col_tile=1024 if vec else 256, block=rb, chunk=0, resident=0,
                partials=-(-T // rb), lane_axis=0)


def want_spectrum_form(T, N, x_stride=None, m_stride=None, has_mask=True, misalign=None):
    mis = misalign or {}
    xs, ms = N if x_stride is None else x_stride, N if m_stride is None else m_stride
    vec = _vec(N, [xs] + ([ms] if has_mask else []), [mis.get("X", 0)] + ([mis.get("M", 0)] if has_mask else []))
    return dict(load_bytes=16 if vec else 4, col_tile=COLS, block=BINS, chunk=CHUNK, resident=int(T <= CHUNK),
                partials=-(-(T // 2) // BINS), lane_axis=0)


def want_affine_form(outer, S, inner, x_strides=None, o_strides=None, misalign=None):
    mis = misalign or {}
    xo, xs = x_strides if x_strides is not None else (S * inner, inner)
    oo, os_ = o_strides if o_strides is not None else (S * inner, inner)
    base = mis.get("x", 0) % 16 == 0 and mis.get("out", 0) % 16 == 0 and (outer == 1 or (xo % 4 == 0 and oo % 4 == 0))
    axis = 0
    if base and inner % 4 == 0 and (S == 1 or (xs % 4 == 0 and os_ % 4 == 0)):
        axis = 1
    elif base and inner == 1 and S % 4 == 0 and xs == 1 and os_ == 1:
        axis = 2
    return dict(load_bytes=16 if axis else 4, col_tile=0, block=1024, chunk=0, resident=0, partials=0, lane_axis=axis)


# ---------------------------------------------------------------- the sweep
def sweep():
    """One case per T of SWEEP_T - N walks SWEEP_N (period 9), the layout LAYOUTS (period 4), the mask kind moves on
    after every four cases (period 12), so that every (mask, layout) pair occurs and neither is a function of N - and two more per T of BOUNDARY_T with N in {32, 64},
    where the 16-byte forms run: an aligned column slice (``slice4``) with every mask kind, and a dense table."""
    cases = [dict(T=T, N=SWEEP_N[k % 9], mask=MASKS[(k // 4) % 3], layout=LAYOUTS[k % 4])
             for k, T in enumerate(SWEEP_T)]
    for j, T in enumerate(BOUNDARY_T):
        cases.append(dict(T=T, N=64, mask=MASKS[j % 3], layout="slice4"))
        cases.append(dict(T=T, N=32, mask=MASKS[(j + 1) % 3], layout=("dense", "slice4")[j % 2]))
    for k, c in enumerate(cases):
        c["seed"] = k
    return cases


def case_id(c):
    return f"T{c['T']}-N{c['N']}-{c['mask']}-{c['layout']}"


def sweep_table(case):
    """``(X, M or None)`` fp32 numpy: counts with a planted wave; ``gaps``: 10 % invalid; ``column``: column 0 as well."""
    T, N = case["T"], case["N"]
    g = np.random.default_rng(1000 + case["seed"])
    t = np.arange(T)[:, None]
    rate = g.uniform(3, 30, (1, N)) * (1.0 + 0.5 * np.sin(2 * np.pi * t / 7.0 + g.uniform(0, 6, (1, N))))
    X = g.poisson(rate).astype(np.float32)
    if case["mask"] == "none":
        return X, None
    M = (g.random((T, N)) >= 0.10).astype(np.float32)
    if case["mask"] == "column":
        M[:, 0] = 0.0
    return X, M


def place(a, layout, device, pad=8):
    """``a`` [T, N] on ``device`` as a dense tensor, a column slice of a wider one (row stride N + pad) that starts 12
    bytes (``slice``) or 16 bytes (``slice4``: on the 16-byte grid) into its row, or a dense tensor one float off the
    16-byte grid."""
    a = torch.as_tensor(a, dtype=torch.float32)
    T, N = a.shape
    if layout == "dense":
        return a.to(device).contiguous()
    if layout in ("slice", "slice4"):
        c0 = 3 if layout == "slice" else 4
        big = torch.full((T, N + pad), float("nan"), dtype=torch.float32, device=device)
        big[:, c0:c0 + N] = a.to(device)
        return big[:, c0:c0 + N]
    flat = torch.full((T * N + 1,), float("nan"), dtype=torch.float32, device=device)
    flat[1:] = a.to(device).reshape(-1)
    return flat[1:].view(T, N)


def layout_args(case):
    """The strides and misalignment ``place`` produces, for the form queries."""
    N = case["N"]
    if case["layout"] == "slice":
        return dict(x_stride=N + 8, m_stride=N + 8, misalign={"X": 12, "M": 12})
    if case["layout"] == "slice4":
        return dict(x_stride=N + 8, m_stride=N + 8)
    if case["layout"] == "off16":
        return dict(misalign={"X": 4, "M": 4})
    return dict()
