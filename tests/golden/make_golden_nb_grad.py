"""Writes the fixture of tests/test_fit_host.py from the reference checkout (Flow-TimesNet, ``src/timesnet_forecast``):
inputs, the loss the reference's own ``losses.negative_binomial_nll`` returned on them and the gradients its fp32
autograd left in ``rate.grad`` / ``dispersion.grad``.  Run once, with the reference checkout's root as argument:

    python tests/golden/make_golden_nb_grad.py REFERENCE_ROOT

nb_grad_cases.npz   <case>:y / rate / disp / mask (absent: none) / loss / g_rate / g_disp, and ``cases`` (the names)
min_sigma_cases.npz <case>:values / mask (absent: none) / global / median / per_series: what ``train._masked_std``
                    returned for both methods (tests/test_fit_forms_table.py)

Inputs: log rate ~ U(-6, 6), y ~ Poisson(rate) with every seventh + 0.37, dispersion log-uniform in the case's band.
The band just above the default floor ``min_sigma = 1e-3`` is where fp32 autograd loses the dispersion gradient.
``special`` plants a NaN y, an inf rate (both outside the mask and inside it) and negative y: the reference's loss is
then NaN (ll * 0) and its gradient is NaN at the planted elements.
"""
from __future__ import annotations

import importlib
import math
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent

CASES = {          # name: (shape, dispersion band, mask: "none" | "float" | "bool" | "allfalse")
    "floor_none": ((4, 16, 16), (1e-3, 1e-2), "none"),
    "mid_float": ((4, 16, 15), (1e-2, 1.0), "float"),
    "high_bool": ((3, 7, 5), (1.0, 100.0), "bool"),
    "floor_allfalse": ((2, 5, 3), (1e-3, 1e-2), "allfalse"),
    "special": ((3, 7, 8), (1e-3, 1e-2), "bool"),
}


def draw(shape, band, g):
    lo, hi = math.log(band[0]), math.log(band[1])
    disp = torch.exp(torch.rand(shape, generator=g) * (hi - lo) + lo)
    rate = torch.exp(torch.rand(shape, generator=g) * 12.0 - 6.0)
    y = torch.poisson(rate, generator=g)
    y.view(-1)[::7] += 0.37
    mask = torch.rand(shape, generator=g) >= 0.2
    return y, rate, disp, mask


def main(ref_root: Path) -> None:
    sys.path.insert(0, str(ref_root / "src"))
    losses = importlib.import_module("timesnet_forecast.losses")
    g = torch.Generator().manual_seed(20241)
    arrays = {"cases": np.array(list(CASES))}
    for name, (shape, band, kind) in CASES.items():
        y, rate, disp, full = draw(shape, band, g)
        mask = {"none": None, "float": full.float() * 2.5, "bool": full, "allfalse": torch.zeros(shape, dtype=torch.bool)}[kind]
        if name == "special":
            mask[0, 0, 0], mask[0, 0, 1], mask[1, 2, 3], mask[1, 2, 4] = False, True, False, True
            y[0, 0, 0] = y[0, 0, 1] = float("nan")
            rate[1, 2, 3] = rate[1, 2, 4] = float("inf")
            y[2, 1, :4] = torch.tensor([-1.0, -0.5, -3.0, -1e-3])
            mask[2, 1, :4] = True
        rate, disp = rate.clone().requires_grad_(), disp.clone().requires_grad_()
        loss = losses.negative_binomial_nll(y, rate, disp, mask)
        loss.backward()
        arrays.update({f"{name}:y": y.numpy(), f"{name}:rate": rate.detach().numpy(), f"{name}:disp": disp.detach().numpy(),
                       f"{name}:loss": np.float32(loss.item()), f"{name}:g_rate": rate.grad.numpy(),
                       f"{name}:g_disp": disp.grad.numpy()})
        if mask is not None:
            arrays[f"{name}:mask"] = mask.numpy()
        print(f"{name}  loss {loss.item():.6f}  |g_disp| max {float(disp.grad.abs().nan_to_num().max()):.3e}")
    out = HERE / "nb_grad_cases.npz"
    np.savez_compressed(out, **arrays)
    print(f"{out.name}  {out.stat().st_size} bytes")


def main_min_sigma(ref_root: Path) -> None:
    train = importlib.import_module("timesnet_forecast.train")
    g = torch.Generator().manual_seed(20242)
    T, N = 57, 9
    values = (torch.randn(T, N, generator=g) * torch.linspace(0.5, 40.0, N) + torch.linspace(-3.0, 900.0, N)).numpy()
    mask = (torch.rand(T, N, generator=g) >= 0.3).float().numpy()
    mask[:, 4] = 0.0                                             # a series with no valid point
    mask[:, 6] = 0.0
    mask[11, 6] = 1.0                                            # and one with a single point
    cases = {"dense": (values, None), "masked": (values, mask), "even": (values[:, :8], mask[:, :8]),
             "all_masked": (values[:5], np.zeros((5, N), dtype=np.float32)),
             "empty": (np.zeros((0, 4), dtype=np.float32), None), "one_series": (values[:, :1], mask[:, :1])}
    arrays = {"cases": np.array(list(cases))}
    for name, (v, m) in cases.items():
        glob, none = train._masked_std([v], [m], method="global")
        med, per = train._masked_std([v], [m], method="per_series_median")
        assert none is None
        arrays.update({f"{name}:values": v, f"{name}:global": np.float64(glob), f"{name}:median": np.float64(med),
                       f"{name}:per_series": np.zeros(v.shape[1]) if per is None else per})
        if m is not None:
            arrays[f"{name}:mask"] = m
        print(f"{name}  global {glob:.6f}  median {med:.6f}")
    out = HERE / "min_sigma_cases.npz"
    np.savez_compressed(out, **arrays)
    print(f"{out.name}  {out.stat().st_size} bytes")


if __name__ == "__main__":
    main(Path(sys.argv[1]).resolve())
    main_min_sigma(Path(sys.argv[1]).resolve())
