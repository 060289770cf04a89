"""What tests/test_nb_sample_host.py, tests/test_gpu_sample.py and tests/golden/make_golden_sample.py share: a numpy
mirror of the sampler's uniforms (written from the contract in include/flowtimes.h, independently of score.py), the
fixtures and the tie rule both backends are held to."""
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden"
FIXTURES = ("std_vector", "std_scalar", "tiny", "large")
TIE_REL, TIE_ABS = 1e-6, 1e-13      # a near tie: F(k*) or F(k* - 1) within max(TIE_REL min(u, 1 - u), TIE_ABS) of u
TIE_CAP = {"std_vector": 1e-3, "std_scalar": 1e-3, "tiny": 1e-3, "large": 0.15}

_cache = {}


def philox_numpy(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on uint64 arrays that hold 32-bit words."""
    M = np.uint64(0xFFFFFFFF)
    c0, c1, c2, c3 = (np.asarray(c, np.uint64) & M for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = np.uint64(k0) & M, np.uint64(k1) & M
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2      # below 2^64: no wrap
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M, (k1 + np.uint64(0xBB67AE85)) & M
    return c0, c1, c2, c3


def uniforms_numpy(S, shape, seed, offset):
    """u[s, e] of the contract, fp64 [S, *shape]."""
    n = int(np.prod(shape))
    e = np.arange(n, dtype=np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    out = np.empty((S, n), np.float64)
    for s in range(S):
        words = philox_numpy(e & np.uint64(0xFFFFFFFF), e >> np.uint64(32), np.uint64(s >> 2), np.uint64(offset),
                             seed & 0xFFFFFFFF, seed >> 32)
        out[s] = (words[s & 3].astype(np.float64) + 0.5) * 2.0 ** -32
    return out.reshape((S,) + tuple(shape))


def load(name):
    if name not in _cache:
        with np.load(GOLDEN / f"nbs_{name}.npz") as z:
            _cache[name] = {k: z[k] for k in z.files}
        for v in _cache[name].values():
            v.setflags(write=False)
    return _cache[name]


def band(u):
    return np.maximum(TIE_REL * np.minimum(u, 1.0 - u), TIE_ABS)


def check_samples(X, z, tag):
    """X == k_star draw for draw; at a recorded near tie the neighbouring integer on the tie's side is allowed too,
    and near ties are at most TIE_CAP of the fixture.  Returns the number of near ties."""
    X = np.asarray(X, np.float64)
    k = z["k_star"].astype(np.float64)
    up, down = z["tie_up"], z["tie_down"]
    assert np.array_equal(z["tie"], up | down)
    ties = int(z["tie"].sum())
    assert ties <= TIE_CAP[tag] * k.size, (tag, ties, k.size)
    ok = (X == k) | (up & (X == k + 1.0)) | (down & (X == k - 1.0))
    assert X.shape == k.shape and bool(ok.all()), (tag, int((~ok).sum()), np.argwhere(~ok)[:4].tolist(),
                                                   X[~ok][:4].tolist(), k[~ok][:4].tolist())
    return ties
