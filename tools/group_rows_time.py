"""Times ``ftn_group_sum_rows`` (``score.group_sums(..., axis=1, backend="hip")``) on sample paths in the pipeline
layout, one series per batch row, with the 9 stores of tests/golden/series_ids.json tiled along B and Poisson(4)
counts.

Shape A, [200, 8192, 28, 1] with the 9 stores and a total - the largest B for which the route without the kernel
exists - four things in one process:
  (a) ``group_sums(x, groups, axis=1)``;
  (b) that route: ``squeeze`` / ``permute`` -> ``.contiguous()`` -> ``group_sums`` along the last axis -> permute back
      (a view), every pass counted;
  (c) ``clone()`` of the samples, the achievable-bandwidth yardstick (its read half is the floor of (a));
  (d) once, untimed: the bit-equality of (a), (b) and the torch backend on one path.
Shape B, [200, 32768, 28, 1] with the 9 stores only (a total would pass the chunk limit): (a) and (c).
The timed variants are alternated round by round, device events around windows of at least 0.3 s after a warm-up, the
median of 3 rounds.  Per variant: the time per call, the bytes it has to move and bytes / time.  Fails without a GPU.

    python tools/group_rows_time.py --out profiles/group_rows_time.json
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import __graft_entry__ as ge  # noqa: E402
from group_time import HBM_PEAK, ROUNDS, alternated  # noqa: E402

SHAPES = (("A", (200, 8192, 28, 1), True), ("B", (200, 32768, 28, 1), False))    # [P, B, H, N], with a total


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "group_rows_time.json"))
    ap.add_argument("--paths", type=int, default=SHAPES[0][1][0])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("group_rows_time: no GPU; nothing is measured without one")
    ftn = ge.load_package()
    sc, rt = ftn.score, ftn.runtime
    dev = torch.device("cuda:0")
    ids = json.loads((ROOT / "tests" / "golden" / "series_ids.json").read_text(encoding="utf-8"))["ids"]
    out_rows = []
    for label, (_, B, H, N), total in SHAPES:
        P = args.paths
        sg = sc.SeriesGroups.from_ids([ids[b % len(ids)] for b in range(B)], device=dev)
        sg = sg.with_total() if total else sg
        G = sg.n_groups
        g = torch.Generator(device=dev).manual_seed(B)
        x = torch.poisson(torch.full((P, B, H, N), 4.0, device=dev), generator=g)
        elems = x.numel()

        def rows_call():
            return sc.group_sums(x, sg, backend="hip", axis=1)

        def transposed():                                       # [P,B,H,1] -> [P,H,B] copy -> [P,H,G] -> [P,G,H,1] view
            t = sc.group_sums(x.squeeze(-1).permute(0, 2, 1).contiguous(), sg, backend="hip")
            return t.permute(0, 2, 1).unsqueeze(-1)

        fns = {"group_sums_axis1": rows_call, "clone": lambda: x.clone()}
        row = {"shape_name": label, "shape": [P, B, H, N], "groups": "9 stores + total" if total else "9 stores", "G": G,
               "members": int(sg.order.numel()), "chunks": sg.n_chunks, "rounds": ROUNDS,
               "form": rt.group_sum_rows_form(sc._group_slabs(x, 1), sg.offsets_host)}
        with torch.inference_mode():
            a = rows_call()
            assert sc._last_group_entry == "ftn_group_sum_rows"
            same = {"torch_backend_one_path": torch.equal(a[0], sc.group_sums(x[0], sg, backend="torch", axis=0))}
            if B <= sc.GROUP_NMAX:
                fns["transpose_copy_route"] = transposed
                same["transpose_copy_route"] = torch.equal(a, transposed())
            del a
            times, counts = alternated(fns)
        row["bit_equal"] = same
        row["calls_per_window"] = counts
        moved = {"group_sums_axis1": 4 * (elems + elems // B * G), "clone": 8 * elems,
                 "transpose_copy_route": 4 * (3 * elems + elems // B * G)}
        for name, (us, us_min) in times.items():
            row[name] = {"us": us, "us_min": us_min, "bytes": moved[name], "bytes_per_s": moved[name] / (us * 1e-6),
                         "share_of_hbm_peak": moved[name] / (us * 1e-6) / HBM_PEAK}
        row["axis1_over_clone_read_half"] = times["group_sums_axis1"][0] / (times["clone"][0] / 2)
        if "transpose_copy_route" in times:
            row["axis1_over_transpose_copy_route"] = times["group_sums_axis1"][0] / times["transpose_copy_route"][0]
        out_rows.append(row)
        print(json.dumps(row), flush=True)
        del x
        torch.cuda.empty_cache()
    Path(args.out).write_text(json.dumps({"device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK,
                                          "rows": out_rows}, indent=1) + "\n")


if __name__ == "__main__":
    main()
