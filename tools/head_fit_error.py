"""Writes profiles/head_fit_error.json from a run of the head-refit tests on the device: the ``FIT_ERR`` lines of
tests/test_gpu_fit.py (largest error as a fraction of its bound, per case), its ``FIT_ADAM`` lines (five Adam steps
against the fp64-driven ones) and the sup-norm errors tests/test_fit_host.py prints for the golden cases.

    python tools/head_fit_error.py --out profiles/head_fit_error.json

The ``adam5`` figures are what ``test_five_adam_steps_against_fp64_gradients`` asserts against; on a first run, before
they exist, that test fails and its printed figures are still recorded.
"""
from __future__ import annotations

import argparse
import json
import re
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "head_fit_error.json"))
    args = ap.parse_args()
    import torch

    cmd = [sys.executable, "-m", "pytest", "-q", "-s", "-p", "no:cacheprovider", "-m", "gpu or not gpu",
           str(ROOT / "tests" / "test_gpu_fit.py"), str(ROOT / "tests" / "test_fit_host.py")]
    text = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True).stdout
    out = {"bound": "|err| <= 4 2^-24 |g| + 2^-36 (log1p(alpha mu) + dpsi) / alpha^2, times the scale 1 / valid",
           "device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
           "fraction_of_bound": [], "head_nll_vs_fp64_autograd": {},
           "adam5": {}, "golden_sup_norm_error_vs_40_digits": []}
    for m in re.finditer(r"FIT_ERR (.*?): fraction of the bound: g_rate ([\d.]+) g_disp ([\d.]+) loss ([\d.]+)", text):
        out["fraction_of_bound"].append({"case": m[1], "g_rate": float(m[2]), "g_disp": float(m[3]), "loss": float(m[4])})
    for m in re.finditer(r"FIT_ERR head_nll (N=\d+): .*? bound ([\d.]+)", text):
        out["head_nll_vs_fp64_autograd"][m[1]] = {"fraction_of_composed_bound": float(m[2])}
    for m in re.finditer(r"FIT_ADAM (N=\d+): .*? run ([\d.e+-]+), between two fp64-driven runs ([\d.e+-]+)", text):
        out["adam5"][m[1]] = {"diff": float(m[2]), "d0": float(m[3])}
    seen = {}
    for m in re.finditer(r"(\w+): sup-norm error ours ([\d.e+-]+) reference (\S+)", text):
        seen.setdefault(m[1], []).append({"fit": float(m[2]), "reference_fp32_autograd": m[3]})
    for case, (rate, disp) in ((k, v) for k, v in seen.items() if len(v) == 2):
        out["golden_sup_norm_error_vs_40_digits"].append({"case": case, "g_rate": rate, "g_disp": disp})
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print(text[-1500:])
    print(json.dumps(out["adam5"]), json.dumps(out["head_nll_vs_fp64_autograd"]))


if __name__ == "__main__":
    main()
