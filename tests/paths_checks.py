"""An independent numpy statement of what ``score.path_summary`` computes (include/flowtimes.h, "summarising sample
paths"), the shapes the path-summary tests share, and the comparisons they make.

Per element (b, h', n): v[p] the window sum (fp64, one rounding to fp32) or window maximum (a NaN stays) of path p;
x = np.sort(v) (NaN last, as torch.sort); quantile q = x[min(max(ceil(q P), 1), P) - 1]; mean = sum x / P;
crps = (A P - G) / P^2 with A = sum |x - yw|, G = sum_i (2 i - P - 1) x(i), in fp64 and rounded once."""
import math

import numpy as np

PATHS = [1, 2, 3, 5, 16, 17, 63, 64, 65, 100, 128, 257, 1024]
SHAPES = [(2, 6, 8), (3, 7, 5), (1, 4, 260), (2, 130, 4)]          # [B, H, N]
LEVELS = [0.05, 0.5, 0.9]
LEVELS11 = [0.01, 0.05, 0.1, 0.25, 0.4, 0.5, 0.6, 0.75, 0.9, 0.95, 0.99]


def windows(H):
    """None, 2 where it divides H, and H."""
    return [None] + ([2] if H % 2 == 0 else []) + [H]


def ranks(levels, P):
    return [min(max(math.ceil(float(q) * P), 1), P) for q in levels]


def padded(P):
    pp = 2
    while pp < P:
        pp *= 2
    return pp


def form(P, vec_ok):
    """The form name ``runtime.path_summary_form`` must give: registers up to 64 padded paths (16-byte accesses only up
    to 16), an LDS tile of min(64, 16384 / PP) columns above."""
    pp = padded(P)
    if pp <= 64:
        return f"reg{pp}/{'vec4' if vec_ok and pp <= 16 else 'scalar'}"
    return f"lds{pp}x{min(64, 16384 // pp)}/{'vec4' if vec_ok else 'scalar'}"


def window_reduce(x, w, reduce):
    """``x`` [..., H, N] fp32 -> [..., H / w, N] fp32."""
    H, N = x.shape[-2:]
    g = x.reshape(x.shape[:-2] + (H // w, w, N))
    if reduce == "max":
        with np.errstate(invalid="ignore"):
            return g.max(axis=-2)                               # np.max propagates NaN
    acc = np.zeros(g.shape[:-2] + (N,), dtype=np.float64)
    with np.errstate(invalid="ignore"):
        for j in range(w):
            acc = acc + g[..., j, :].astype(np.float64)
    return acc.astype(np.float32)


def summary(x, levels, window=None, reduce="sum", y=None):
    """The oracle: a dict with ``quantiles``, ``mean``, ``sorted``, and with ``y`` also ``crps``, ``yw`` and ``scale``
    (fp64: A / P + |G| / P^2, the magnitude the CRPS rounding is measured at); ``mean_scale`` likewise."""
    x = np.asarray(x, dtype=np.float32)
    P, B, H, N = x.shape
    w = 1 if window is None else int(window)
    v = window_reduce(x, w, reduce)
    xs = np.sort(v, axis=0)
    xd = xs.astype(np.float64)
    out = {"sorted": xs, "quantiles": xs[[r - 1 for r in ranks(levels, P)]] if len(levels) else xs[:0]}
    with np.errstate(invalid="ignore", over="ignore"):
        out["mean"] = (xd.sum(0) / P).astype(np.float32)
        out["mean_scale"] = np.abs(xd).sum(0) / P
        if y is not None:
            yw = window_reduce(np.asarray(y, dtype=np.float32), w, reduce)
            coef = (2.0 * np.arange(1, P + 1, dtype=np.float64) - (P + 1)).reshape(P, 1, 1, 1)
            A, G = np.abs(xd - yw.astype(np.float64)).sum(0), (coef * xd).sum(0)
            out["crps"] = ((A * P - G) / float(P * P)).astype(np.float32)
            out["crps64"] = (A * P - G) / float(P * P)
            out["scale"] = A / P + np.abs(G) / float(P * P)
            out["yw"] = yw
    return out


def same(a, b):
    """Equal values, NaN equal to NaN: bit equality for everything but the sign of a zero."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(a, b, equal_nan=True))


def within_ulp(got, want64, scale):
    """|got - want| <= one fp32 ulp at ``scale`` (fp64 arrays), element by element; NaN must meet NaN.  The fp64
    accumulation error (<= P 2^-53 relative to the same scale) is orders below the final fp32 rounding, which is half
    an ulp of the RESULT <= half an ulp at ``scale``; one ulp leaves room for a rounding that lands on the other side."""
    got, want64 = np.asarray(got, dtype=np.float64), np.asarray(want64, dtype=np.float64)
    nan = np.isnan(want64)
    if not np.array_equal(np.isnan(got), nan):
        return False
    with np.errstate(invalid="ignore"):
        ulp = np.spacing(np.abs(scale).astype(np.float32)).astype(np.float64)
        ok = (got == want64) | (np.abs(got - want64) <= ulp)
    return bool(ok[~nan].all())


def counts(g, shape, lam):
    """Poisson counts as fp32: many ties at a low rate."""
    return g.poisson(lam, shape).astype(np.float32)


def big_counts(g, shape, window):
    """Integer values whose window sums stay just below 2^24, so every sum is exact in fp32."""
    top = (1 << 24) // max(int(window), 1) - 1
    return (top - g.integers(0, 1000, shape)).astype(np.float32)
