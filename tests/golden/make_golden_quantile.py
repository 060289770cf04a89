"""Writes the fixtures of tests/test_nb_quantile_host.py and tests/test_gpu_quantile.py with scipy as the yardstick
(``scipy.special.betainc`` in fp64; ``scipy.stats.nbinom.ppf`` for a first guess of the quantile, then moved until
scipy's own CDF brackets the level).  The tests read only the committed ``.npz`` files; scipy is needed here alone.

    python tests/golden/make_golden_quantile.py

nbq_<case>.npz   rate, disp (fp32 [B,H,N]), levels (fp64 [Q]), k_star (fp64 [Q,B,H,N]: the smallest k with
                 F(k) >= q), F_k = F(k_star), F_km1 = F(k_star - 1) (0 where k_star = 0), y (fp32 [B,H,N]: half of it
                 a quantile, half a random count, a few entries negative or fractional), F_y = F(floor(max(y, 0)))
nbq_poisson.npz  rate (fp32), disp = 1e-8 everywhere (the clamp), levels, ppf = scipy.stats.poisson.ppf(levels, rate)

The parameterisation is the scorer's: alpha = max(disp, 1e-8), mu = max(rate, 1e-8) in fp32, then in fp64
r = 1 / alpha, p = 1 / (1 + alpha mu), F(k) = I_p(r, k + 1).  Every element and level must satisfy
F(k* - 1) < q <= F(k*); near ties (F(k*) or F(k* - 1) within 1e-6 min(q, 1 - q) of q) may be at most 0.1 % of a
fixture's element-levels.  Both are asserted before a file is written.  In the ``large`` regime the pmf at a
quantile falls to 1e-6 and below, where that band catches a fair share of all levels by itself, so its tied elements
are drawn again from the same regime until none is left: the fixture holds the elements whose answer is unambiguous.
"""
from __future__ import annotations

from pathlib import Path

import numpy as np
from scipy import special, stats

HERE = Path(__file__).resolve().parent
STD_LEVELS = (0.025, 0.1, 0.5, 0.9, 0.975)
TIE = 1e-6

CASES = {   # name: (shape, (mu_lo, mu_hi), (alpha_lo, alpha_hi), levels, seed)
    "scalar": ((3, 7, 5), (1e-3, 2e3), (1e-3, 5.0), STD_LEVELS, 0),
    "vector": ((4, 24, 36), (1e-3, 2e3), (1e-3, 5.0), STD_LEVELS, 0),
    "pipeline": ((5, 7, 1), (1e-3, 2e3), (1e-3, 5.0), STD_LEVELS, 0),
    "large": ((2, 4, 8), (1e4, 1e6), (1e-3, 1.0), STD_LEVELS, 1),
    "tiny": ((2, 4, 8), (1e-6, 1e-2), (1e-3, 5.0), (0.025, 0.5, 0.975, 0.999, 0.99999), 2),
}


def params(rate, disp):
    al = np.maximum(disp.astype(np.float32), np.float32(1e-8)).astype(np.float64)
    mu = np.maximum(rate.astype(np.float32), np.float32(1e-8)).astype(np.float64)
    return 1.0 / al, 1.0 / (1.0 + al * mu)


def cdf(k, r, p):
    """F(k) for integer-valued k; 0 below 0."""
    return np.where(k >= 0, special.betainc(r, np.maximum(k, 0.0) + 1.0, p), 0.0)


def quantile(q, r, p):
    k = np.maximum(np.nan_to_num(stats.nbinom.ppf(q, r, p), nan=0.0), 0.0)
    for _ in range(64):                                         # ppf may be a step off: move until the CDF brackets q
        up, down = cdf(k, r, p) < q, (k > 0) & (cdf(k - 1.0, r, p) >= q)
        if not (up.any() or down.any()):
            break
        k = np.where(up, k + 1.0, np.where(down, k - 1.0, k))
    return k


def near_tie(Fk, Fkm1, q):
    band = TIE * min(q, 1.0 - q)
    return (np.abs(Fk - q) <= band) | (np.abs(Fkm1 - q) <= band)


def main() -> None:
    for name, (shape, (mlo, mhi), (alo, ahi), levels, seed) in CASES.items():
        g = np.random.default_rng(seed)
        rate = np.exp(g.uniform(np.log(mlo), np.log(mhi), shape)).astype(np.float32)
        disp = np.exp(g.uniform(np.log(alo), np.log(ahi), shape)).astype(np.float32)
        lv = np.asarray(levels, np.float64)
        for _ in range(200):
            r, p = params(rate, disp)
            k_star = np.stack([quantile(q, r, p) for q in lv])
            F_k = np.stack([cdf(k, r, p) for k in k_star])
            F_km1 = np.stack([cdf(k - 1.0, r, p) for k in k_star])
            tied = np.any(np.stack([near_tie(F_k[i], F_km1[i], q) for i, q in enumerate(lv)]), 0)
            if name != "large" or not tied.any():
                break
            # a pmf of 1e-6 and less makes a near tie the rule: draw the tied elements again (same regime)
            rate = np.where(tied, np.exp(g.uniform(np.log(mlo), np.log(mhi), shape)), rate).astype(np.float32)
            disp = np.where(tied, np.exp(g.uniform(np.log(alo), np.log(ahi), shape)), disp).astype(np.float32)
        ties = 0
        for i, q in enumerate(lv):
            assert np.all(F_km1[i] < q) and np.all(q <= F_k[i]), (name, q)
            ties += int(near_tie(F_k[i], F_km1[i], q).sum())
        assert ties <= 1e-3 * k_star.size, (name, ties, k_star.size)
        assert k_star.max() < 2 ** 24
        pick = g.integers(0, len(lv), shape)
        y = np.take_along_axis(k_star, pick[None], 0)[0]
        counts = stats.nbinom.rvs(r, p, random_state=g).astype(np.float64)
        y = np.where(g.random(shape) < 0.5, y, np.minimum(counts, 2.0 ** 24 - 1))
        flat = y.reshape(-1)
        flat[0] = -3.0
        flat[1 % flat.size] += 0.5 if flat.size > 1 else 0.0
        if flat.size > 4:
            flat[3] = -0.25
            flat[4] += 0.75
        y = y.astype(np.float32)                                # counts below 2^24 are exact in fp32
        F_y = cdf(np.floor(np.maximum(y.astype(np.float64), 0.0)), r, p)
        out = HERE / f"nbq_{name}.npz"
        np.savez_compressed(out, rate=rate, disp=disp, levels=lv, k_star=k_star, F_k=F_k, F_km1=F_km1, y=y, F_y=F_y)
        print(f"{out.name}  shape {shape}  k* max {k_star.max():.0f}  near ties {ties}/{k_star.size}  "
              f"{out.stat().st_size} bytes")
    g = np.random.default_rng(3)
    shape = (2, 4, 8)
    rate = np.exp(g.uniform(np.log(1e-2), np.log(1e3), shape)).astype(np.float32)
    lv = np.asarray(STD_LEVELS, np.float64)
    ppf = np.stack([stats.poisson.ppf(q, rate.astype(np.float64)) for q in lv])
    out = HERE / "nbq_poisson.npz"
    np.savez_compressed(out, rate=rate, disp=np.full(shape, 1e-8, np.float32), levels=lv, ppf=ppf)
    print(f"{out.name}  ppf max {ppf.max():.0f}  {out.stat().st_size} bytes")


if __name__ == "__main__":
    main()
