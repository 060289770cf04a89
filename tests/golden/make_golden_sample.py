"""Writes the fixtures of tests/test_nb_sample_host.py and tests/test_gpu_sample.py with scipy as the yardstick
(``scipy.special.betainc`` in fp64; ``scipy.stats.nbinom.ppf`` for a first guess, then moved until scipy's own CDF
brackets the uniform).  The tests read only the committed ``.npz`` files; scipy is needed here alone.

    python tests/golden/make_golden_sample.py

nbs_<case>.npz  rate, disp (fp32 [B,H,N]), seed (uint64), offset, S, k_star (int32 [S,B,H,N]: the smallest k with
                F(k) >= u[s, e]), tie_up / tie_down / tie (bool [S,B,H,N]: F(k_star), F(k_star - 1), either within
                max(1e-6 min(u, 1 - u), 1e-13) of u; the 1e-13 is the kernels' NBQ_CF_EPS, below which the CDF is not
                resolved)

The uniforms are not stored: the tests recompute them (tests/nbs_checks.py, the contract of include/flowtimes.h).  The
parameterisation and the regimes are those of make_golden_quantile.py.  Every draw must satisfy
F(k* - 1) < u <= F(k*); near ties may be at most 0.1 % of a fixture's draws (std, tiny) or 15 % (large, where the pmf
at the answer is about 1e-6, the band itself).  Both are asserted before a file is written.
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
import nbs_checks as ns  # noqa: E402
from make_golden_quantile import cdf, params, quantile  # noqa: E402

SEED, OFFSET = (0x9E3779B9 << 32) | 0x7F4A7C15, 3
CASES = {   # name: (shape, S, (mu_lo, mu_hi), (alpha_lo, alpha_hi), numpy seed)
    "std_vector": ((4, 24, 36), 16, (1e-3, 2e3), (1e-3, 5.0), 0),
    "std_scalar": ((3, 7, 5), 5, (1e-3, 2e3), (1e-3, 5.0), 0),
    "large": ((2, 4, 8), 16, (1e4, 1e6), (1e-3, 1.0), 1),
    "tiny": ((2, 4, 8), 16, (1e-6, 1e-2), (1e-3, 5.0), 2),
}


def main() -> None:
    for name, (shape, S, (mlo, mhi), (alo, ahi), seed) in CASES.items():
        g = np.random.default_rng(seed)
        rate = np.exp(g.uniform(np.log(mlo), np.log(mhi), shape)).astype(np.float32)
        disp = np.exp(g.uniform(np.log(alo), np.log(ahi), shape)).astype(np.float32)
        r, p = params(rate, disp)
        u = ns.uniforms_numpy(S, shape, SEED, OFFSET)
        k_star = quantile(u, r[None], p[None])
        F_k, F_km1 = cdf(k_star, r[None], p[None]), cdf(k_star - 1.0, r[None], p[None])
        assert np.all(F_km1 < u) and np.all(u <= F_k), name
        assert k_star.max() < 2 ** 24
        b = ns.band(u)
        up, down = np.abs(F_k - u) <= b, np.abs(F_km1 - u) <= b
        ties = int((up | down).sum())
        assert ties <= ns.TIE_CAP[name] * k_star.size, (name, ties, k_star.size)
        out = HERE / f"nbs_{name}.npz"
        np.savez_compressed(out, rate=rate, disp=disp, seed=np.uint64(SEED), offset=np.int64(OFFSET), S=np.int64(S),
                            k_star=k_star.astype(np.int32), tie_up=up, tie_down=down, tie=up | down)
        print(f"{out.name}  shape {shape} S {S}  k* max {k_star.max():.0f}  near ties {ties}/{k_star.size}  "
              f"{out.stat().st_size} bytes")


if __name__ == "__main__":
    main()
