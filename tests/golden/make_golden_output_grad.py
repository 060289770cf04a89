"""Writes the fixtures of tests/test_output_fit_host.py from the reference checkout (Flow-TimesNet,
``src/timesnet_forecast``): the reference ``TimesNet`` at the tiny configuration of tests/test_gpu_fit.py's
``_tiny_model`` (L 24, H 4, d_model 16, 2 blocks), its zero-initialised parameters woken up as the drop-in fixtures do,
one batch, the reference's own loss (``losses.negative_binomial_nll``) and what its autograd leaves in the six tensors
of the output side.  Run once, with the reference checkout's root as argument:

    python tests/golden/make_golden_output_grad.py REFERENCE_ROOT

output_grad_n<N>.npz   N in {1, 5}: the config, the state_dict, x / y / mask, the input of ``forecast_time_proj``
                       (a forward pre-hook) as seq [B, L, D], the loss and the six fp32 gradients

Before a fixture is written the reference's gradients are held against the fp64 composition of
tests/output_fit_oracle.py within ONE composed bound (the test allows two: both sides are fp32 evaluations of one
function); a seed that misses is skipped and reported, and with no seed inside the bound nothing is written."""
from __future__ import annotations

import importlib
import json
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, str(HERE.parents[1]))

L, H = 24, 4
CFG = dict(input_len=L, pred_len=H, d_model=16, d_ff=32, n_layers=2, k_periods=3, kernel_set=[(3, 3), (5, 5)],
           dropout=0.0, activation="gelu", mode="direct", use_checkpoint=False)


def make_case(ref_model, ref_losses, ftn, oracle, N: int, seed: int):
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(0)
    want = ref_model.TimesNet(**CFG).eval()
    with torch.no_grad():
        want(torch.rand(2, L, N, generator=g) + 1.0)
        for p in want.parameters():                          # wake up the zero-initialised parameters
            if float(p.abs().sum()) == 0.0:
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
    t = torch.arange(L, dtype=torch.float32).view(1, L, 1)
    x = torch.rand(4, L, N, generator=g) + 1.5 + torch.sin(2 * torch.pi * t / 6.0)
    y = torch.poisson(torch.full((4, H, N), 2.0), generator=g)
    mask = (torch.rand(4, H, N, generator=g) >= 0.2).float()
    seen = {}
    hook = want.forecast_time_proj.register_forward_pre_hook(lambda mod, args: seen.update(seq=args[0].detach().clone()))
    rate, disp = want(x)
    hook.remove()
    loss = ref_losses.negative_binomial_nll(y, rate, disp, mask > 0)
    loss.backward()
    with_grad = sorted(k for k, p in want.named_parameters() if p.grad is not None and bool(p.grad.abs().sum() > 0))
    assert set(oracle.NAMES) <= set(with_grad), with_grad     # (the backbone gets gradients too: not recorded)
    named = dict(want.named_parameters())
    grads = [named[k].grad.detach().clone() for k in oracle.NAMES]
    seq = seen["seq"].permute(0, 2, 1).contiguous()          # the module reads [B, D, L]
    assert seq.shape == (4, L, CFG["d_model"])

    # the fp64 composition from the same seq, on our model's head inputs
    sd = {k: v.detach().clone() for k, v in want.state_dict().items()}
    with torch.no_grad():
        torch.manual_seed(1)
        mine = ftn.models.TimesNet(**CFG).eval()
        mine(x)
        mine.load_state_dict(sd, strict=True)
    _, tail, hist, late, floor = mine.head_inputs(x)
    params = [dict(mine.named_parameters())[k] for k in oracle.NAMES]
    loss64, want64, bounds = oracle.grads_and_bounds(ftn.fit, seq, params, tail, hist, y, mask > 0, late, floor,
                                                     mine.min_sigma)
    frac = oracle.fraction(grads, want64, bounds)
    lo, hi = float(disp.min()), float(disp.max())
    print(f"N={N} seed={seed}: reference against fp64, fraction of one bound {frac:.4f}; dispersion in "
          f"[{lo:.3f}, {hi:.3f}]; loss {float(loss):.7f} (fp64 {float(loss64):.7f})")
    if frac > 1.0:
        return None, frac
    arrays = {"config_json": np.asarray(json.dumps(CFG)), "x": x.numpy(), "y": y.numpy(), "mask": mask.numpy(),
              "seq": seq.numpy(), "loss": loss.detach().numpy(), "fraction_of_bound": np.asarray(frac)}
    arrays.update({f"sd:{k}": v.numpy() for k, v in sd.items()})
    arrays.update({f"grad:{k}": v.numpy() for k, v in zip(oracle.NAMES, grads)})
    return arrays, frac


def main(ref_root: Path) -> None:
    import __graft_entry__ as ge
    import output_fit_oracle as oracle

    sys.path.insert(0, str(ref_root / "src"))
    ref_model = importlib.import_module("timesnet_forecast.models.timesnet")
    ref_losses = importlib.import_module("timesnet_forecast.losses")
    ftn = ge.load_package()
    for N in (1, 5):
        tried = []
        for seed in range(1, 9):
            arrays, frac = make_case(ref_model, ref_losses, ftn, oracle, N, seed)
            tried.append(frac)
            if arrays is not None:
                np.savez_compressed(HERE / f"output_grad_n{N}.npz", **arrays)
                print(f"output_grad_n{N}.npz  seed {seed}")
                break
        else:
            raise SystemExit(f"N={N}: no seed within one bound, fractions {tried}: nothing written")


if __name__ == "__main__":
    main(Path(sys.argv[1]))
