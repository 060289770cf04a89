"""An independent numpy statement of what ``score.group_sums`` computes (include/flowtimes.h, "series groups"), the
shapes and group layouts the series-group tests share, and the comparisons they make.

Per row x[0..N) and group of members i_0 .. i_{m-1}: the members in chunks of 32 consecutive ones, a chunk's sum in
fp64 left to right from +0.0, the chunk sums added in ascending order in fp64, one rounding to fp32."""
import json
from pathlib import Path

import numpy as np

import paths_checks as pc  # noqa: F401  (the path-summary oracle the end-to-end tests apply to the totals)

CHUNK = 32
NS = [1, 3, 4, 5, 33, 64, 193, 260]
ROWS = [1, 7, 67]                                               # 67: above every tile height (<= 64), a partial last tile
FIXTURE = Path(__file__).resolve().parent / "golden" / "series_ids.json"


def fixture():
    """``(ids, [(store, size), ..])`` of tests/golden/series_ids.json."""
    d = json.loads(FIXTURE.read_text(encoding="utf-8"))
    return d["ids"], [(k, int(v)) for k, v in d["stores"]]


def group_sum(x, members):
    """The oracle: ``x`` [..., N] fp32 and a list of member lists -> [..., G] fp32."""
    x = np.asarray(x, dtype=np.float32)
    rows = x.reshape(-1, x.shape[-1])
    out = np.zeros((rows.shape[0], len(members)), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for g, m in enumerate(members):
            total = np.zeros(rows.shape[0], dtype=np.float64)
            for k in range(0, len(m), CHUNK):
                acc = np.zeros(rows.shape[0], dtype=np.float64)
                for i in m[k:k + CHUNK]:
                    acc = acc + rows[:, i].astype(np.float64)
                total = total + acc
            out[:, g] = total.astype(np.float32)
    return out.reshape(x.shape[:-1] + (len(members),))


def chunks(members):
    return sum((len(m) + CHUNK - 1) // CHUNK for m in members)


def tile_rows(N, n_chunks):
    """The header's rule: a row takes 4 (N + N / 32 + 1) + 8 n_chunks bytes; 32 KiB of them, at most 64, at least 1."""
    return max(1, min(64, 32768 // (4 * (N + N // 32 + 1) + 8 * n_chunks)))


def form(N, stride, misalign, n_chunks):
    """The form name ``runtime.group_sum_form_of`` must give."""
    vec = N % 4 == 0 and stride % 4 == 0 and misalign % 16 == 0
    return f"{'vec4' if vec else 'scalar'}/t{tile_rows(N, n_chunks)}"


def layouts(N):
    """name -> member lists over N series."""
    out = {"all": [list(range(N))],
           "own": [[i] for i in range(N)],
           "mod3": [[n for n in range(N) if n % 3 == g] for g in range(3)],          # order is not the identity
           "some": [[n for n in range(N) if n % 4 == 1], [n for n in range(N) if n % 4 == 2]] if N > 2 else [[0]],
           "overlap": [list(range(0, (2 * N + 2) // 3)), list(range(N - 1, N // 3 - 1, -1)), list(range(N))],
           "empty": [list(range(N // 2)), [], list(range(N // 2, N)), []]}
    if N >= 161:
        out["sizes"] = [list(range(0, 31)), list(range(31, 63)), list(range(63, 96)), list(range(96, 161))]
    return out


def values(g, shape, members):
    """kind -> fp32 array of ``shape`` [..., N]: Poisson counts, counts whose totals stay just below 2^24, signed
    normals, and counts with a NaN in one series and an inf in another."""
    N = shape[-1]
    top = (1 << 24) // max(max(len(m) for m in members), 1) - 1
    special = g.poisson(3.0, shape).astype(np.float32)
    special[..., N // 2] = np.nan
    if N > 1:
        special[..., N - 1] = np.inf
        special.reshape(-1, N)[::2, N - 1] = -np.inf
    return {"counts": g.poisson(1.5, shape).astype(np.float32),
            "big": (top - g.integers(0, min(1000, top), shape)).astype(np.float32),
            "normal": (g.standard_normal(shape) * 100.0).astype(np.float32),
            "special": special}


def bits_equal(a, b):
    """Equal bit for bit (the sign of a zero included), a NaN matching any NaN."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != np.float32 or b.dtype != np.float32:
        return False
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan]))
