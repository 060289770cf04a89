"""Writes the fixtures of tests/test_score_host.py and tests/test_gpu_score.py from the reference checkout
(Flow-TimesNet, ``src/timesnet_forecast``): inputs, and what the reference's own ``losses.negative_binomial_nll`` /
``negative_binomial_mask``, ``utils.metrics.smape_mean`` / ``wsmape_grouped`` and ``train._eval_metrics`` returned on
them.  Run once, with the reference checkout's root as argument:

    python tests/golden/make_golden_score.py REFERENCE_ROOT

score_nll_<case>.npz   y, rate, disp, mask (absent: none), nll, valid, smape (smape_mean on the masked arrays)
score_eval_<case>.npz  b<i>:x / y / mask / ids / rate / disp of every batch, names (the id strings), use_loss_mask,
                       nll, smape (_eval_metrics), wsmape, wsmape_weighted (+ weight_names, weight_values)

Inputs are ones on which the reference stays finite: rate = exp(U(-4, 8)), dispersion = exp(U(log 1e-6, 2)),
y ~ Poisson(min(rate, 1e4)), a 20 % random mask.
"""
from __future__ import annotations

import importlib
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent


def draw(shape, g):
    rate = torch.exp(torch.rand(shape, generator=g) * 12.0 - 4.0)
    lo = float(np.log(1e-6))
    disp = torch.exp(torch.rand(shape, generator=g) * (2.0 - lo) + lo)
    y = torch.poisson(rate.clamp(max=1e4), generator=g)
    mask = torch.rand(shape, generator=g) >= 0.2
    return y, rate, disp, mask


NLL_CASES = {          # name: (shape, mask: "full" | "none" | "float" | rank-1 "b" | rank-2 "bh")
    "full": ((4, 12, 10), "full"),
    "none": ((3, 7, 5), "none"),
    "float": ((2, 5, 8), "float"),
    "bh": ((4, 24, 37), "bh"),
    "b": ((5, 7, 1), "b"),
}


class Recorded(torch.nn.Module):
    """A model that returns the recorded (rate, dispersion) of its calls in turn."""

    def __init__(self, outs, input_len):
        super().__init__()
        self.outs, self.i, self.input_len = outs, 0, input_len

    def forward(self, xb, **kw):
        out = self.outs[self.i]
        self.i += 1
        return out


def main(ref_root: Path) -> None:
    sys.path.insert(0, str(ref_root / "src"))
    losses = importlib.import_module("timesnet_forecast.losses")
    metrics = importlib.import_module("timesnet_forecast.utils.metrics")
    train = importlib.import_module("timesnet_forecast.train")
    g = torch.Generator().manual_seed(20240)
    for name, (shape, kind) in NLL_CASES.items():
        y, rate, disp, full = draw(shape, g)
        mask = {"full": full, "none": None, "float": full.float() * 2.5, "bh": full[:, :, 0], "b": full[:, 0, 0]}[kind]
        nll = losses.negative_binomial_nll(y, rate, disp, mask)
        valid = losses.negative_binomial_mask(y, rate, disp, mask)
        w = valid.to(y.dtype)
        smape = metrics.smape_mean((y * w).numpy().reshape(-1, shape[2]), (rate * w).numpy().reshape(-1, shape[2]))
        assert bool(torch.isfinite(nll))
        arrays = {"y": y.numpy(), "rate": rate.numpy(), "disp": disp.numpy(), "nll": np.float32(nll.item()),
                  "valid": valid.numpy(), "smape": np.float64(smape)}
        if mask is not None:
            arrays["mask"] = mask.numpy()
        out = HERE / f"score_nll_{name}.npz"
        np.savez_compressed(out, **arrays)
        print(f"{out.name}  nll {float(nll):.6f}  smape {smape:.6f}  {out.stat().st_size} bytes")

    EVAL_CASES = {     # name: (B, L, H, N, per-sample ids, use_loss_mask, id strings)
        "shared": (3, 8, 6, 5, False, True, ["a_1", "a_2", "b_1", "b_2", "c_1"]),
        "pipeline": (8, 8, 5, 1, True, True, ["s_x", "s_y", "t_x", "u_x"]),
        "nomask": (2, 8, 4, 8, False, False, [f"{'pq'[i % 2]}_{i}" for i in range(8)]),
    }
    for name, (B, L, H, N, per_sample, use_mask, names) in EVAL_CASES.items():
        batches, outs, arrays = [], [], {}
        # _eval_metrics stacks one column per id: every id gets the same number of (b, n) columns over the run
        balanced = torch.arange(len(names)).repeat(3 * B * N // len(names))[torch.randperm(3 * B * N, generator=g)]
        for i in range(3):
            y, rate, disp, mask = draw((B, H, N), g)
            x = torch.rand(B, L, N, generator=g)
            if per_sample:
                ids = balanced[i * B * N:(i + 1) * B * N].reshape(B, N)
                batches.append((x, y, mask.float(), None, None, None, ids))
                arrays[f"b{i}:ids"] = ids.numpy()
            else:
                batches.append((x, y, mask.float()))
            outs.append((rate, disp))
            arrays.update({f"b{i}:x": x.numpy(), f"b{i}:y": y.numpy(), f"b{i}:mask": mask.float().numpy(),
                           f"b{i}:rate": rate.numpy(), f"b{i}:disp": disp.numpy()})
        dev = torch.device("cpu")
        res = train._eval_metrics(Recorded(outs, L), batches, dev, "direct", names, H, use_loss_mask=use_mask)
        ws = train._eval_wsmape(Recorded(outs, L), batches, dev, "direct", names, H, use_loss_mask=use_mask)
        # the weighted variant: the columns _eval_metrics stacks, given to wsmape_grouped with weights
        tg = {i: [] for i in range(len(names))}
        pr = {i: [] for i in range(len(names))}
        for (batch, (rate, disp)) in zip(batches, outs):
            y, m = batch[1], batch[2]
            valid = losses.negative_binomial_mask(y, rate, disp, (m > 0) if use_mask else None).to(y.dtype)
            ids = batch[6] if per_sample else torch.arange(N).unsqueeze(0).expand(B, -1)
            for b in range(B):
                for n in range(N):
                    tg[int(ids[b, n])].append((y * valid)[b, :, n].numpy())
                    pr[int(ids[b, n])].append((rate * valid)[b, :, n].numpy())
        Y, P = train._stack_series_columns(tg, len(names)), train._stack_series_columns(pr, len(names))
        stores = sorted({s.split("_", 1)[0] for s in names})
        weights = {st: float(1 + k) for k, st in enumerate(stores)}
        arrays.update({"names": np.array(names), "use_loss_mask": np.bool_(use_mask), "nll": np.float64(res["nll"]),
                       "smape": np.float64(res["smape"]), "wsmape": np.float64(ws),
                       "wsmape_weighted": np.float64(metrics.wsmape_grouped(Y, P, names, weights)),
                       "wsmape_check": np.float64(metrics.wsmape_grouped(Y, P, names, None)),
                       "weight_names": np.array(stores), "weight_values": np.array([weights[s] for s in stores])})
        out = HERE / f"score_eval_{name}.npz"
        np.savez_compressed(out, **arrays)
        print(f"{out.name}  nll {res['nll']:.6f}  smape {res['smape']:.6f}  wsmape {ws:.6f}  {out.stat().st_size} bytes")


if __name__ == "__main__":
    main(Path(sys.argv[1]).resolve())
