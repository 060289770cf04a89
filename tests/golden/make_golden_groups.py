"""Writes tests/golden/series_ids.json, the fixture of the series-group tests, from the reference checkout
(Flow-TimesNet): the series names of ``data/sample_submission.csv`` (its header without the date column; a name is
``"store_menu"``), and the stores the reference's grouping rule (``utils/metrics.py``, ``wsmape_grouped``: the text
before the first ``"_"``, stores in first-appearance order) makes of them, with their sizes.  Run once, with the
reference checkout's root as argument:

    python tests/golden/make_golden_groups.py REFERENCE_ROOT

series_ids.json   {"ids": [193 names], "stores": [[name, size], ..]}
"""
from __future__ import annotations

import csv
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent


def main() -> None:
    root = Path(sys.argv[1])
    with open(root / "data" / "sample_submission.csv", newline="", encoding="utf-8-sig") as f:
        ids = next(csv.reader(f))[1:]
    sizes = {}
    for name in ids:
        store = name.split("_", 1)[0]
        sizes[store] = sizes.get(store, 0) + 1                  # a dict keeps first-appearance order
    assert len(ids) == len(set(ids)) and all("_" in s for s in ids)
    (HERE / "series_ids.json").write_text(
        json.dumps({"ids": ids, "stores": [[k, v] for k, v in sizes.items()]}, ensure_ascii=False, indent=0) + "\n",
        encoding="utf-8")
    print(len(ids), "series,", len(sizes), "stores:", list(sizes.values()))


if __name__ == "__main__":
    main()
