"""Pins what the torch backends of ``score.nb_quantiles`` and ``score.nb_sample`` computed on the CPU at commit
0c1f81e ("Store totals on the device: series-group sums of paths and forecasts"), the last one with a search loop
of its own in each of them, so that tests/test_nb_quantile_host.py can hold the shared search to those bits.

    python tests/golden/make_golden_nb_torch.py [--all OUT.npz]

nb_torch_parent.npz  q_<case> (fp32 [Q,B,H,N]) and qflag_<case> (int32) of ``_nb_quantiles_torch`` on nbq_<case>.npz at
                     its own levels, case in scalar, pipeline, large, tiny; s_<case> (fp32 [S,B,H,N]) and sflag_<case>
                     of ``nb_sample(backend="torch")`` on nbs_<case>.npz at its own S, seed and offset, case in
                     std_scalar, tiny, large; and the same for ``edge``: one row of NaN, inf, out-of-range and below-eps
                     parameters (edge_rate, edge_disp are stored beside the results).

The two larger fixtures (nbq_vector, nbs_std_vector) are not stored; ``--all`` writes them too, into a file of the
caller's choice, for a comparison by hand.  Run it only at a commit whose results are meant to be the pin.
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parents[1]))
import __graft_entry__ as ge  # noqa: E402

Q_CASES = ("scalar", "pipeline", "large", "tiny")
S_CASES = ("std_scalar", "tiny", "large")
EDGE_LEVELS = (0.025, 0.5, 0.975)
EDGE_S, EDGE_SEED, EDGE_OFFSET = 5, 11, 2


def edge_inputs():
    """[1,1,12]: NaN, +-inf, a rate whose quantiles pass 2^24, parameters below eps, zero, negative, and plain ones."""
    nan, inf = float("nan"), float("inf")
    rate = [nan, 1.0, inf, 1.0, 1e8, 3e7, 1e-12, 0.0, -1.0, 5.0, 2.5, 1e3]
    disp = [1.0, nan, 1.0, inf, 1.0, 1e-3, 1.0, 1e-12, 0.5, -1.0, 0.0, 4.0]
    return tuple(torch.tensor(v, dtype=torch.float32).view(1, 1, -1) for v in (rate, disp))


def quantiles(sc, rate, disp, levels):
    out, flag = sc._nb_quantiles_torch(rate, disp, [float(q) for q in levels], 1e-8)
    return out.numpy(), np.int32(int(flag))


def samples(sc, rate, disp, S, seed, offset):
    flag = torch.zeros(1, dtype=torch.int32)
    out = sc.nb_sample(rate, disp, S, seed, offset, backend="torch", flag=flag)
    return out.numpy(), np.int32(int(flag))


def compute(sc, q_cases=Q_CASES, s_cases=S_CASES):
    res = {}
    for name in q_cases:
        with np.load(HERE / f"nbq_{name}.npz") as z:
            res[f"q_{name}"], res[f"qflag_{name}"] = quantiles(sc, torch.from_numpy(z["rate"]),
                                                               torch.from_numpy(z["disp"]), z["levels"])
    for name in s_cases:
        with np.load(HERE / f"nbs_{name}.npz") as z:
            rate, disp = torch.from_numpy(z["rate"]), torch.from_numpy(z["disp"])
            res[f"s_{name}"], res[f"sflag_{name}"] = samples(sc, rate, disp, int(z["S"]), int(z["seed"]), int(z["offset"]))
    rate, disp = edge_inputs()
    res["edge_rate"], res["edge_disp"] = rate.numpy(), disp.numpy()
    res["q_edge"], res["qflag_edge"] = quantiles(sc, rate, disp, EDGE_LEVELS)
    res["s_edge"], res["sflag_edge"] = samples(sc, rate, disp, EDGE_S, EDGE_SEED, EDGE_OFFSET)
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--all", default=None, help="also run nbq_vector and nbs_std_vector and write everything here")
    args = ap.parse_args()
    sc = ge.load_package().score
    if args.all:
        np.savez_compressed(args.all, **compute(sc, Q_CASES + ("vector",), S_CASES + ("std_vector",)))
        return
    out = HERE / "nb_torch_parent.npz"
    res = compute(sc)
    np.savez_compressed(out, **res)
    for k, v in res.items():
        if k.startswith(("q_", "s_")):
            print(f"{k}  shape {v.shape}  NaN {int(np.isnan(v).sum())}  flag {int(res[k.replace('_', 'flag_', 1)])}")
    print(f"{out.name}  {out.stat().st_size} bytes")


if __name__ == "__main__":
    main()
