"""Writes the fixtures of tests/test_recursive_forecast.py and tests/test_gpu_recursive.py from the reference checkout
(Flow-TimesNet, ``src/timesnet_forecast``): its own ``TimesNet(mode="recursive")`` built on each case's config, the
state_dict it held after its zero-initialised parameters (heads, context coefficients, late bias) were woken up, the
inputs, and what its own ``predict.forecast_recursive_batch`` returned.  Run once, with the reference checkout's root as
argument:

    python tests/golden/make_golden_recursive.py REFERENCE_ROOT

recursive_<case>.npz   x, kw:<input>, sd:<state_dict key>, rate, disp, periods (the last step's)
"""
from __future__ import annotations

import importlib
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))


def _np(v):
    return v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


def main(ref_root: Path) -> None:
    import test_recursive_forecast as t

    sys.path.insert(0, str(ref_root / "src"))
    tsn = importlib.import_module("timesnet_forecast.models.timesnet")
    predict = importlib.import_module("timesnet_forecast.predict")
    for name, (cfg, _, _) in t.CASES.items():
        x, kw, H, g = t.case_inputs(name)
        with torch.no_grad():
            torch.manual_seed(0)
            model = tsn.TimesNet(**cfg).eval()
            model(x, **{k: v for k, v in kw.items() if k != "y_mark"})
            for p in model.parameters():                      # wake up the zero-initialised parameters
                if float(p.detach().abs().sum()) == 0.0:
                    p.copy_(t.WAKE * torch.randn(p.shape, generator=g))
            rate, disp = predict.forecast_recursive_batch(model, x, H, **kw)
            periods = model.period_selector.last_selected_periods.tolist()
        arrays = {"x": _np(x), "rate": _np(rate), "disp": _np(disp), "periods": np.asarray(periods, np.int64)}
        arrays.update({f"kw:{k}": _np(v) for k, v in kw.items()})
        arrays.update({f"sd:{k}": _np(v) for k, v in model.state_dict().items()})
        out = HERE / f"recursive_{name}.npz"
        np.savez_compressed(out, **arrays)
        print(f"{out.name}  H={H}  periods {periods}  {out.stat().st_size} bytes")


if __name__ == "__main__":
    main(Path(sys.argv[1]).resolve())
