"""Writes profiles/output_fit_error.json from a run of the output-refit tests on the device: the ``OUTFIT_ERR`` lines of
tests/test_gpu_output_fit.py and tests/test_output_fit_host.py (largest error as a fraction of its bound, per case) and
the ``OUTFIT_ADAM`` lines (five Adam steps of ``fit.refit_output`` against the fp64-driven ones):

  diff   the largest parameter difference to the fp64-driven run
  d0     the same between two fp64-driven runs with the batch rows reversed: the reference point, which never
         involves the code under test

    python tools/output_fit_error.py --out profiles/output_fit_error.json

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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "output_fit_error.json"))
    args = ap.parse_args()
    import torch

    cmd = [sys.executable, "-m", "pytest", "-q", "-s", "-p", "no:cacheprovider", "-m", "gpu or not gpu",
           str(ROOT / "tests" / "test_gpu_output_fit.py"), str(ROOT / "tests" / "test_output_fit_host.py")]
    text = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True).stdout
    out = {"bound": "grid: (B D + 2) 2^-24 sum |dH seq|; output_nll: the composed bounds of tests/output_fit_oracle.py",
           "device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
           "grid_fraction_of_bound": [], "output_nll_vs_fp64_autograd": {}, "reference_anchor": {}, "adam5": {}}
    for m in re.finditer(r"OUTFIT_ERR grid (\d+) (B=\d+ L=\d+ S=\d+ D=\d+): .*?: dW_t ([\d.]+) db_t ([\d.]+)", text):
        out["grid_fraction_of_bound"].append({"case": int(m[1]), "shape": m[2], "dW_t": float(m[3]), "db_t": float(m[4])})
    for m in re.finditer(r"OUTFIT_ERR output_nll (N=\d+): .*?: time projection ([\d.]+) heads ([\d.]+)", text):
        out["output_nll_vs_fp64_autograd"][m[1]] = {"time_projection": float(m[2]), "heads": float(m[3])}
    for m in re.finditer(r"OUTFIT_ERR reference anchor (N=\d+): .*? fp64 ([\d.]+), the reference against fp64 ([\d.]+), "
                         r"ours against the reference \(allowed 2\) ([\d.]+)", text):
        out["reference_anchor"][m[1]] = {"ours_vs_fp64": float(m[2]), "reference_vs_fp64": float(m[3]),
                                         "ours_vs_reference": float(m[4])}
    for m in re.finditer(r"OUTFIT_ADAM (N=\d+): .*? run ([\d.e+-]+), between two fp64-driven runs ([\d.e+-]+)", text):
        out["adam5"][m[1]] = {"diff": float(m[2]), "d0": float(m[3])}
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print(text[-2500:])
    print(json.dumps(out["adam5"]), json.dumps(out["output_nll_vs_fp64_autograd"]))


if __name__ == "__main__":
    main()
