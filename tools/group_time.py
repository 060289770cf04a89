"""Times ``ftn_group_sum`` (``score.group_sums(..., backend="hip")``) on samples [200, 64, 28, 512] with the 9 stores
of tests/golden/series_ids.json tiled to 512 series, and with those 9 plus a total, beside three things on the same
tensors in the same run: ``index_add_`` in fp32, the one-hot matmul in fp32, and a ``clone()`` of the samples as the
achievable-bandwidth yardstick.  One process, the variants alternated round by round, device events around windows
of at least 0.3 s after a warm-up, the median of 3 rounds.  Per variant: the time per call, the bytes it has to move
(group sums: 4 (rows N + rows G); clone: 8 rows N, a read and a write) and bytes / time.  Fails without a GPU.

    python tools/group_time.py --out profiles/group_time.json
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

SHAPE = (200, 64, 28, 512)   # [P, B, H, N]
HBM_PEAK = 8.0e12            # bytes / s, the datasheet figure
WINDOW_S = 0.3
ROUNDS = 3


def window(fn, n):
    """Microseconds per call over n back-to-back calls between two device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / n


def alternated(fns):
    """``{name: (median, min)}`` microseconds per call: a warm-up, a count per variant that fills WINDOW_S, then ROUNDS
    rounds that take every variant in turn."""
    counts = {}
    for name, fn in fns.items():
        fn()
        torch.cuda.synchronize()
        counts[name] = max(1, math.ceil(WINDOW_S * 1e6 / window(fn, 2)))
    seen = {name: [] for name in fns}
    for _ in range(ROUNDS):
        for name, fn in fns.items():
            seen[name].append(window(fn, counts[name]))
    return {name: (statistics.median(v), min(v)) for name, v in seen.items()}, counts


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "group_time.json"))
    ap.add_argument("--paths", type=int, default=SHAPE[0])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("group_time: no GPU; nothing is measured without one")
    ftn = ge.load_package()
    sc, rt = ftn.score, ftn.runtime
    dev = torch.device("cuda:0")
    P, (B, H, N) = args.paths, SHAPE[1:]
    ids = json.loads((ROOT / "tests" / "golden" / "series_ids.json").read_text(encoding="utf-8"))["ids"]
    stores = sc.SeriesGroups.from_ids([ids[n % len(ids)] for n in range(N)], device=dev)
    g = torch.Generator(device=dev).manual_seed(N)
    x = torch.poisson(torch.full((P, B, H, N), 4.0, device=dev), generator=g)
    x2 = x.view(-1, N)
    rows = x2.shape[0]
    out_rows = []
    for label, sg in (("9 stores", stores), ("9 stores + total", stores.with_total())):
        G = sg.n_groups
        order = sg.order.long()
        owner = torch.repeat_interleave(torch.arange(G, device=dev), torch.from_numpy(sg.offsets_host).diff().to(dev))
        onehot = torch.zeros(N, G, device=dev).index_put_((order, owner), torch.ones((), device=dev), accumulate=True)
        if sorted(sg.order_host.tolist()) == list(range(N)):    # a partition: index_add_ by the owner of every column
            col_owner = torch.empty(N, dtype=torch.long, device=dev)
            col_owner[order] = owner

            def index_add():
                return torch.zeros(rows, G, device=dev).index_add_(1, col_owner, x2)
        else:                                                   # overlapping groups: gather the members first

            def index_add():
                return torch.zeros(rows, G, device=dev).index_add_(1, owner, x2.index_select(1, order))
        with torch.inference_mode():
            hip = sc.group_sums(x, sg, backend="hip")
            same = torch.equal(hip[0], sc.group_sums(x[0], sg, backend="torch"))     # one path: the torch backend is fp64
            exact = torch.equal(hip.view(rows, G), index_add()) and torch.equal(hip.view(rows, G), x2 @ onehot)
            del hip
            times, counts = alternated({
                "group_sums": lambda: sc.group_sums(x, sg, backend="hip"),
                "index_add": index_add,
                "onehot_matmul": lambda: x2 @ onehot,
                "clone": lambda: x.clone()})
        moved = 4 * (rows * N + rows * G)
        row = {"groups": label, "shape": [P, B, H, N], "G": G, "members": int(sg.order.numel()), "chunks": sg.n_chunks,
               "form": rt.group_sum_form(x2, sg.offsets_host), "equal_to_torch_backend": same,
               "counts_equal_index_add_and_matmul": exact, "calls_per_window": counts, "rounds": ROUNDS}
        for name, (us, us_min) in times.items():
            nbytes = 8 * rows * N if name == "clone" else moved
            row[name] = {"us": us, "us_min": us_min, "bytes": nbytes, "bytes_per_s": nbytes / (us * 1e-6),
                         "share_of_hbm_peak": nbytes / (us * 1e-6) / HBM_PEAK}
        row["group_sums_over_clone_read_half"] = times["group_sums"][0] / (times["clone"][0] / 2)
        out_rows.append(row)
        print(json.dumps(row), flush=True)
    Path(args.out).write_text(json.dumps({"device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK,
                                          "rows": out_rows}, indent=1) + "\n")


if __name__ == "__main__":
    main()
