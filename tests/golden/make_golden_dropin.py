"""Writes the fixtures of tests/test_dropin_reference.py and tests/test_predict_pipeline_dropin.py from the reference
checkout (Flow-TimesNet, ``src/timesnet_forecast``): what its own ``TimesNet`` was built with, the state_dict it
held, the inputs it was called on and what it returned.  Run once, with the reference checkout's root as argument:

    python tests/golden/make_golden_dropin.py REFERENCE_ROOT

dropin_<case>.npz   the cases of test_dropin_reference.py (configs and inputs are defined there)
pipeline_predict_once.npz   the model calls of the reference's ``predict_once`` on its own data file
                            data/test/TEST_00.csv and artifacts written with its own writers
"""
from __future__ import annotations

import importlib
import json
import pickle
import shutil
import sys
import tempfile
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))


def _np(v):
    return v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


def _pack(prefix, tensors):
    return {f"{prefix}{k}": _np(v) for k, v in tensors.items()}


# ------------------------------------------------------------------------------------------------ shell cases
def make_shell_cases(ref_src: Path) -> None:
    import test_dropin_reference as t

    sys.path.insert(0, str(ref_src))
    ref = importlib.import_module("timesnet_forecast.models.timesnet")
    for name, (cfg, wake) in t.CASES.items():
        x, kw, g = t.case_inputs(name)
        with torch.no_grad():
            torch.manual_seed(0)
            want = ref.TimesNet(**cfg).eval()
            want(x, **kw)
            for p in want.parameters():                      # wake up the zero-initialised heads
                if float(p.detach().abs().sum()) == 0.0:
                    p.copy_(wake * torch.randn(p.shape, generator=g))
            rate, disp = want(x, **kw)
            periods = want.period_selector.last_selected_periods.tolist()
            torch.manual_seed(0)
            fresh = ref.TimesNet(**cfg).eval()
            rate0, disp0 = fresh(x, **kw)
        arrays = {"x": _np(x), "rate": _np(rate), "disp": _np(disp), "periods": np.asarray(periods, np.int64),
                  "rate_init": _np(rate0), "disp_init": _np(disp0)}
        arrays.update(_pack("kw:", kw))
        arrays.update(_pack("sd:", want.state_dict()))
        arrays.update(_pack("init_sd:", fresh.state_dict()))
        np.savez_compressed(HERE / f"dropin_{name}.npz", **arrays)
        print(f"dropin_{name}.npz  periods {periods}")


# ------------------------------------------------------------------------------------------------ predict_once
DATE, SID, TARGET = "영업일자", "영업장명_메뉴명", "매출수량"


def _write_artifacts(ref, tmp_path, ids, static_np, data_csv, P):
    cfgmod, io_utils, meta_utils = (ref("timesnet_forecast.config"), ref("timesnet_forecast.utils.io"),
                                    ref("timesnet_forecast.utils.metadata"))
    tsn = ref("timesnet_forecast.models.timesnet")
    IN, OUT, MODEL = P.INPUT_LEN, P.PRED_LEN, P.MODEL
    art = tmp_path / "artifacts"
    art.mkdir()
    n = len(ids)

    # a reference model in its trained shape: warm-up as train.py does, widen the id table, wake the heads
    torch.manual_seed(0)
    model = tsn.TimesNet(channels_last=False, use_checkpoint=False, **MODEL)
    with torch.no_grad():
        model(torch.zeros(1, IN, 1), series_static=torch.from_numpy(static_np[:1]), series_ids=torch.tensor([n - 1]))
        g = torch.Generator().manual_seed(7)
        for p in model.parameters():
            if float(p.abs().sum()) == 0.0:
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
    assert model.series_embedding.num_embeddings == n
    torch.save(model.state_dict(), art / "timesnet.pth")

    tf = cfgmod.TimeFeatureConfig(enabled=False).to_dict()
    names = [f"f{i}" for i in range(static_np.shape[1])]
    with open(art / "scaler.pkl", "wb") as f:
        pickle.dump({"ids": ids, "method": "none", "scaler": None, "static_features": static_np,
                     "feature_names": names, "time_features": {"enabled": False, "feature_dim": 0, "config": tf}}, f)
    schema = io_utils.DataSchema.from_fields({"date": DATE, "id": SID, "target": TARGET},
                                             sources={"date": "override", "id": "override", "target": "override"})
    io_utils.save_schema_artifact(str(art / "schema.json"), schema,
                                  normalization={"method": "none", "per_series": True, "eps": 1e-8})
    window = cfgmod.WindowConfig(input_len=IN, pred_len=OUT, stride=1, short_series_strategy="error", pad_value=0.0)
    meta = meta_utils.MetadataArtifact.from_training(
        window=window, schema=schema,
        time_features={"config": tf, "enabled": False, "feature_dim": 0, "freq": None},
        static_features={"feature_names": names, "feature_dim": static_np.shape[1]})
    meta_utils.save_metadata_artifact(meta, str(art / "metadata.json"))

    test_dir = tmp_path / "test"
    test_dir.mkdir()
    shutil.copy(data_csv, test_dir / "TEST_00.csv")
    cfg = {
        "artifacts": {"dir": str(art), "model_file": "timesnet.pth", "scaler_file": "scaler.pkl",
                      "schema_file": "schema.json", "config_file": "config_used.yaml",
                      "signature_file": "model_signature.json", "metadata_file": "metadata.json"},
        "data": {"test_dir": str(test_dir), "sample_submission": str(tmp_path / "absent.csv"),
                 "fill_missing_dates": False, "date_col": DATE, "id_col": SID, "target_col": TARGET,
                 "time_features": tf, "encoding": "utf-8-sig"},
        "preprocess": {"clip_negative": False, "normalize": "none", "normalize_per_series": True, "eps": 1e-8},
        "train": {"device": "cpu", "matmul_precision": "highest", "channels_last": False, "amp": False,
                  "use_checkpoint": False, "cuda_graphs": False,
                  "val": {"strategy": "holdout", "holdout_days": IN + OUT}},
        "model": dict(MODEL),
        "window": {"input_len": IN, "pred_len": OUT, "stride": 1, "short_series_strategy": "error", "pad_value": 0.0},
        "submission": {"out_path": str(tmp_path / "out" / "submission.csv"), "format": "row_key", "date_col": DATE},
    }
    import yaml
    with open(art / "config_used.yaml", "w", encoding="utf-8") as f:
        yaml.safe_dump({k: cfg[k] for k in ("model", "train", "data", "artifacts", "submission", "preprocess")}, f,
                       allow_unicode=True)
    return cfg


def make_pipeline(ref_root: Path) -> None:
    import pandas as pd
    import test_predict_pipeline_dropin as P

    ref_src = ref_root / "src"
    sys.path.insert(0, str(ref_src))
    ref = importlib.import_module
    predict = ref("timesnet_forecast.predict")
    io_utils = ref("timesnet_forecast.utils.io")
    tsn = ref("timesnet_forecast.models.timesnet")
    data_csv = ref_root / "data" / "test" / "TEST_00.csv"
    raw = pd.read_csv(data_csv, encoding="utf-8-sig")
    ids = sorted({io_utils.normalize_id(v) for v in raw[SID].unique()})      # the ids training would have stored
    assert len(ids) > 100 and raw[DATE].nunique() == P.INPUT_LEN
    static_np = np.random.RandomState(3).randn(len(ids), 4).astype(np.float32)

    rec = {"ctor": None, "calls": []}

    class Recorder(tsn.TimesNet):
        def __init__(self, *a, **kw):
            assert not a
            super().__init__(*a, **kw)
            rec["ctor"] = kw

        def forward(self, x, **kw):
            seen = {"x": x.clone(), "kw": {k: v.clone() for k, v in kw.items()},
                    "sd": {k: v.clone() for k, v in self.state_dict().items()},
                    "id_vocab": self._series_id_vocab,
                    "id_reference": None if self._series_id_reference is None else self._series_id_reference.clone()}
            out = super().forward(x, **kw)
            rec["calls"].append(dict(seen, out=tuple(o.clone() for o in out)))
            return out

    with tempfile.TemporaryDirectory() as td:
        cfg = _write_artifacts(ref, Path(td), ids, static_np, data_csv, P)
        predict.TimesNet = Recorder
        want = pd.read_csv(predict.predict_once(cfg))
    ctor = rec["ctor"]
    json.dumps(ctor)                                     # every constructor argument is a plain value
    warm, *calls = rec["calls"]
    assert len(calls) == 1, len(calls)
    call = calls[0]
    rate, disp = call["out"]
    # what the CSV holds: rate [rows, H, 1] -> one column per series, clipped at 0 ("none" normalisation)
    table = want.iloc[:, 1:].to_numpy(np.float64)
    np.testing.assert_allclose(table, np.clip(_np(rate)[:, :table.shape[0], 0].T.astype(np.float64), 0.0, None),
                               rtol=1e-6, atol=1e-7)
    arrays = {"ctor_json": np.asarray(json.dumps(ctor)), "x": _np(call["x"]), "rate": _np(rate), "disp": _np(disp),
              "warm_x": _np(warm["x"]), "id_reference": _np(call["id_reference"]),
              "id_vocab": np.asarray(call["id_vocab"], np.int64),
              "submission": table, "submission_row_key": np.asarray(want.iloc[:, 0].astype(str).tolist())}
    arrays.update(_pack("kw:", call["kw"]))
    arrays.update(_pack("warm_kw:", warm["kw"]))
    arrays.update(_pack("sd:", call["sd"]))
    np.savez_compressed(HERE / "pipeline_predict_once.npz", **arrays)
    print("pipeline_predict_once.npz", {k: v.shape for k, v in arrays.items() if not k.startswith("sd:")})


if __name__ == "__main__":
    root = Path(sys.argv[1])
    make_shell_cases(root / "src")
    make_pipeline(root)
