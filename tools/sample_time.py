"""Times ``k_nb_sample`` at [256, 96, 512] with S = 1 and S = 16 (device events, warm-up, the median of 20 runs) beside
stock torch ops on the same tensors (``torch.poisson`` of a gamma draw: the gamma-Poisson mixture, S tensors' worth),
and ``forecast_sample_paths`` beside the mean-fed ``forecast_recursive_batch`` at the same batch P B.  The sampler's
cost per draw depends on the data, so each row states its regime as tools/quantile_time.py does.

    python tools/sample_time.py --out profiles/sample_time.json
"""
from __future__ import annotations

import argparse
import json
import math
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import __graft_entry__ as ge  # noqa: E402

SHAPE = (256, 96, 512)
REGIMES = {"fixtures": ((1e-3, 2e3), (1e-3, 5.0)), "counts": ((0.5, 50.0), (0.05, 1.0))}


def timed(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return statistics.median(out), min(out)


def stock(rate, disp, S):
    """S gamma-Poisson draws per element with torch's own samplers."""
    conc = (1.0 / disp).expand(S, *rate.shape)
    gam = torch._standard_gamma(conc) * (rate * disp)
    return torch.poisson(gam)


def forecast_rows(ftn, dev, reps):
    fc = ftn.forecast
    L, N, H, B, P = 96, 64, 24, 4, 16
    cfg = dict(input_len=L, pred_len=4, d_model=64, d_ff=128, n_layers=2, k_periods=3, kernel_set=[(3, 3), (5, 5)],
               dropout=0.0, activation="gelu", mode="recursive", use_checkpoint=False)
    torch.manual_seed(0)
    model = ftn.models.TimesNet(**cfg).eval().to(dev)
    g = torch.Generator().manual_seed(1)
    t = torch.arange(L, dtype=torch.float32).view(1, L, 1)
    x = (torch.rand(B, L, N, generator=g) * 4.0 + 3.0 + 2.0 * torch.sin(2 * torch.pi * t / 12.0)).to(dev)
    with torch.inference_mode():
        model(x)
        for p in model.parameters():
            if float(p.detach().abs().sum()) == 0.0:
                p.copy_((0.1 * torch.randn(p.shape, generator=g)).to(dev))
        xr = x.repeat(P, 1, 1)
        us_mean, _ = timed(lambda: fc.forecast_recursive_batch(model, xr, H), reps, 2)
        us_paths, _ = timed(lambda: fc.forecast_sample_paths(model, x, H, P, seed=1), reps, 2)
    return {"model": {k: cfg[k] for k in ("input_len", "d_model", "n_layers")}, "N": N, "H": H, "B": B, "P": P,
            "forecast_recursive_batch_us": us_mean, "forecast_sample_paths_us": us_paths,
            "embed_backend": model._last_embed_backend, "sample_backend": ftn.score._last_backend,
            "per_step_extra_us": (us_paths - us_mean) / H}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "sample_time.json"))
    args = ap.parse_args()
    ftn = ge.load_package()
    rt = ftn.runtime
    dev = torch.device("cuda:0")
    B, H, N = SHAPE
    rows = []
    for regime, ((mlo, mhi), (alo, ahi)) in REGIMES.items():
        g = torch.Generator(device=dev).manual_seed(B + N)
        u = lambda lo, hi: torch.exp(torch.rand(B, H, N, generator=g, device=dev) * math.log(hi / lo) + math.log(lo))
        rate, disp = u(mlo, mhi), u(alo, ahi)
        for S in (1, 16):
            out = torch.empty(S, B, H, N, device=dev)
            flag = torch.zeros(1, dtype=torch.int32, device=dev)
            reps = 20 if S == 1 else 5
            with torch.inference_mode():
                us, us_min = timed(lambda: rt.nb_sample(rate, disp, S, 1, 0, out=out, flag=flag), reps, 2)
                us_stock, _ = timed(lambda: stock(rate, disp, S), reps, 2)
            n = B * H * N * S
            rows.append({"shape": [B, H, N], "S": S, "regime": regime, "mu": [mlo, mhi], "alpha": [alo, ahi],
                         "form": rt.nb_sample_form(rate, disp), "flag": int(flag), "reps": reps,
                         "k_nb_sample_us": us, "k_nb_sample_us_min": us_min, "k_nb_sample_ns_per_draw": us * 1e3 / n,
                         "torch_gamma_poisson_us": us_stock, "torch_gamma_poisson_ns_per_draw": us_stock * 1e3 / n,
                         "mean_draw": float(out.mean())})
            print(json.dumps(rows[-1]), flush=True)
    fr = forecast_rows(ftn, dev, 5)
    print(json.dumps(fr), flush=True)
    Path(args.out).write_text(json.dumps({"device": torch.cuda.get_device_name(0), "rows": rows, "forecast": fr},
                                         indent=1) + "\n")


if __name__ == "__main__":
    main()
