"""What tests/test_nb_quantile_host.py and tests/test_gpu_quantile.py share: the fixtures of
tests/golden/make_golden_quantile.py and the rules both backends are held to."""
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden"
FIXTURES = ("scalar", "vector", "pipeline", "large", "tiny")
TIE = 1e-6                      # a near tie: F(k*) or F(k* - 1) within TIE min(q, 1 - q) of q
TIE_CAP = 1e-3                  # of a fixture's element-levels at most
U32 = 2.0 ** -24

_cache = {}


def load(name):
    if name not in _cache:
        with np.load(GOLDEN / f"nbq_{name}.npz") as z:
            _cache[name] = {k: z[k] for k in z.files}
        for v in _cache[name].values():
            v.setflags(write=False)
    return _cache[name]


def band(levels):
    lv = np.asarray(levels, np.float64)
    return (TIE * np.minimum(lv, 1.0 - lv)).reshape(-1, 1, 1, 1)


def cdf_error(F, F_ref):
    """max |F - F_ref| / max(min(F_ref, 1 - F_ref), 2^-24)."""
    den = np.maximum(np.minimum(F_ref, 1.0 - F_ref), U32)
    return float((np.abs(np.asarray(F, np.float64) - F_ref) / den).max())


def check_quantiles(Q, z, tag):
    """Q == k_star element for element; at a near tie the neighbouring integer on the tie's side is allowed too, and
    near ties are at most TIE_CAP of the fixture."""
    Q = np.asarray(Q, np.float64)
    k, lv = z["k_star"], z["levels"]
    up = np.abs(z["F_k"] - lv.reshape(-1, 1, 1, 1)) <= band(lv)          # F(k*) barely reaches q: k* + 1 may come out
    down = np.abs(z["F_km1"] - lv.reshape(-1, 1, 1, 1)) <= band(lv)      # F(k* - 1) barely misses q: k* - 1 may
    ties = int((up | down).sum())
    assert ties <= TIE_CAP * k.size, (tag, ties, k.size)
    ok = (Q == k) | (up & (Q == k + 1.0)) | (down & (Q == k - 1.0))
    assert Q.shape == k.shape and bool(ok.all()), (tag, int((~ok).sum()), np.argwhere(~ok)[:4].tolist(),
                                                   Q[~ok][:4].tolist(), k[~ok][:4].tolist())
    return ties


def interval_metrics_numpy(z, valid=None):
    """coverage, pinball, pit_mean in fp64 from the fixture's k_star and F_y."""
    y = z["y"].astype(np.float64)
    valid = np.ones(y.shape, bool) if valid is None else valid
    n = max(int(valid.sum()), 1)
    lv = z["levels"]
    d = y[None] - z["k_star"]
    pin = np.maximum(lv.reshape(-1, 1, 1, 1) * d, (lv.reshape(-1, 1, 1, 1) - 1.0) * d)
    return ((y[None] <= z["k_star"]) & valid).sum((1, 2, 3)) / n, (pin * valid).sum((1, 2, 3)) / n, \
        float((z["F_y"] * valid).sum() / n)
