"""What a row pass costs (DESIGN §4 "Row passes"), three measurements into one JSON:

  bench      the ``bench.py`` headline of this tree and, with ``--parent-tree``, of a checkout of the parent commit (its
             library built, ``--parent-lib``), alternated run by run in child processes: nothing existing moved.
  c2         BASELINE configs[2]'s block (B = 256, L = 336, d_model 64, k = 5) in one pass and in four passes of 64.
  pipeline   the pipeline layout, one series per batch row: 38 600 rows (193 series x 200 paths), L = 28, d_model 128,
             in one pass and in passes of 8 192, with the workspace bytes of each.
The block variants are alternated round by round in one process (``TimesBlock.rows_per_pass``), device events around
windows of at least 0.3 s after a warm-up, the median of 3 rounds; the outputs of the variants are compared bit for
bit once, untimed.  Fails without a GPU.

    python tools/rows_pass_time.py --out profiles/rows_pass_time.json [--parent-tree DIR --parent-lib DIR/.../lib.so]
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import __graft_entry__ as ge  # noqa: E402
from group_time import ROUNDS, alternated  # noqa: E402

KS = [(3, 3), (5, 5), (7, 7)]
BENCH_ARGS = ["--gpus", "1", "--steps", "300", "--warmup", "30"]
BENCH_ROUNDS = 3


def bench_once(tree: Path, lib: str | None) -> dict:
    env = dict(os.environ)
    if lib:
        env["FLOWTIMES_LIB"] = lib
    else:
        env.pop("FLOWTIMES_LIB", None)
    p = subprocess.run([sys.executable, str(tree / "bench.py"), *BENCH_ARGS], cwd=str(tree), env=env, capture_output=True,
                       text=True, timeout=900)
    if p.returncode != 0:
        raise SystemExit(f"bench.py in {tree} failed:\n{p.stdout[-2000:]}{p.stderr[-4000:]}")
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


def block_case(ftn, dev, B, L, C, K, rows):
    """One block at (B, L, C): one pass against passes of ``rows``."""
    T, rt = ftn.models.timesnet, ftn.runtime
    blk = T.TimesBlock(C, KS, 0.0, "gelu", d_ff=4 * C, bottleneck_ratio=4.0)
    sd = ftn.synth.make_inception_params(C, 4 * C, KS, 4.0, seed=0)
    blk.inception.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    blk.period_selector = T.FFTPeriodSelector(K, L)
    blk = blk.eval().to(dev)
    g = torch.Generator(device=dev).manual_seed(B)                    # seeded noise over two planted periods (7 and 4)
    t = torch.arange(L, dtype=torch.float32, device=dev).view(1, L, 1)
    x = (torch.randn(B, L, C, device=dev, generator=g) + 2.0 * torch.sin(2 * torch.pi * t / 7.0)
         + torch.cos(2 * torch.pi * t / 4.0)).contiguous()
    _, plan = blk._packed(dev)
    mg, pxb = rt.selector_bounds(L, K, L, 1)
    ws = lambda n: int(ftn.lib.load().ftn_timesblock_workspace_bytes(plan, n, L, mg, pxb))

    def run(r):
        def fn():
            blk.rows_per_pass = r
            return blk(x)
        return fn

    with torch.inference_mode():
        one = run(None)().clone()
        forms_one, passes_one = blk._last_forms, blk._last_passes
        many = run(rows)().clone()
        forms_many, passes_many = blk._last_forms, blk._last_passes
        blk.check_range()
        times, counts = alternated({"one_pass": run(None), "passes": run(rows)})
        blk.check_range()
    return {"B": B, "L": L, "d_model": C, "k_periods": K, "engine": blk._engine_name(), "rows_per_pass": rows,
            "passes": list(passes_many), "one_pass": {"us": times["one_pass"][0], "us_min": times["one_pass"][1],
                                                      "workspace_bytes": ws(B), "passes": list(passes_one),
                                                      "forms": forms_one},
            "in_passes": {"us": times["passes"][0], "us_min": times["passes"][1], "workspace_bytes": ws(min(B, rows)),
                          "forms": forms_many},
            "passes_over_one_pass": times["passes"][0] / times["one_pass"][0], "bit_equal": torch.equal(one, many),
            "rounds": ROUNDS, "calls_per_window": counts}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "rows_pass_time.json"))
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit (bench.py is run there)")
    ap.add_argument("--parent-lib", default=None, help="its built libflowtimes_hip.so (FLOWTIMES_LIB for those runs)")
    ap.add_argument("--skip-bench", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rows_pass_time: no GPU; nothing is measured without one")
    doc = {"device": torch.cuda.get_device_name(0)}
    if not args.skip_bench:
        trees = {"this": (ROOT, os.environ.get("FLOWTIMES_LIB"))}
        if args.parent_tree:
            trees["parent"] = (Path(args.parent_tree).resolve(), args.parent_lib and str(Path(args.parent_lib).resolve()))
        seen = {k: [] for k in trees}
        extra = {}
        for r in range(BENCH_ROUNDS):
            for name, (tree, lib) in trees.items():
                d = bench_once(tree, lib)
                seen[name].append(d["ms_per_step"])
                extra[name] = {"metric": d.get("metric"), "config": d.get("config")}
                print(f"bench round {r} {name}: {d['ms_per_step']:.4f} ms/step", flush=True)
        med = {k: sorted(v)[len(v) // 2] for k, v in seen.items()}
        doc["bench"] = {"args": BENCH_ARGS, "rounds": BENCH_ROUNDS, "ms_per_step": med, "ms_per_step_rounds": seen,
                        "headline": extra}
        if "parent" in med:
            doc["bench"]["this_over_parent"] = med["this"] / med["parent"]
    ftn = ge.load_package()
    dev = torch.device("cuda:0")
    doc["c2"] = block_case(ftn, dev, 256, 336, 64, 5, 64)
    print("c2:", doc["c2"]["passes_over_one_pass"], flush=True)
    doc["pipeline"] = block_case(ftn, dev, 193 * 200, 28, 128, 5, 8192)
    print("pipeline:", doc["pipeline"]["passes_over_one_pass"], flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
