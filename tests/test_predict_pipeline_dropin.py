"""the mirror ``TimesNet`` as the reference's own inference pipeline drives it, pinned by a fixture
the reference wrote (tests/golden/make_golden_dropin.py).

The reference's ``predict_once`` (predict.py:345-1000) reads ``config_used.yaml``, ``metadata.json``,
``schema.json``, ``scaler.pkl`` and a ``state_dict`` checkpoint, rebuilds ``TimesNet`` with a warm-up
call, resizes the id embedding, ``load_state_dict(strict=True)``, windows ``data/test/TEST_00.csv``
(193 series x 28 days, one series per batch row: ``x[B=193, L=28, N=1]`` with per-sample static
features and ids) and writes a submission CSV.  The fixture holds, from one run of that pipeline on a checkpoint
written by the reference model (all artifacts written with the reference's own writers): the constructor arguments
``predict_once`` passed, its warm-up call, the state the model held and the batch it was called on, what the model
returned and the submission CSV's numbers.  The mirror, driven through the same steps, must return the same."""
import json

import numpy as np
import pytest
import torch

from conftest import GOLDEN

INPUT_LEN, PRED_LEN = 28, 7
MODEL = dict(mode="direct", input_len=INPUT_LEN, pred_len=PRED_LEN, d_model=16, d_ff=32, n_layers=2, k_periods=2,
             kernel_set=[3, 5], dropout=0.0, activation="gelu", bottleneck_ratio=2.0, use_embedding_norm=True,
             id_embed_dim=6, static_proj_dim=5, static_layernorm=True, min_period_threshold=1,
             use_zero_mean_context=True, context_rank=3, context_scale=0.05, use_constant_context_bias=True)


def _part(z, prefix):
    return {k[len(prefix):]: torch.from_numpy(np.array(v)) for k, v in z.items() if k.startswith(prefix)}


def test_predict_once_with_mirror_model(ftn):
    with np.load(GOLDEN / "pipeline_predict_once.npz") as f:
        z = {k: f[k] for k in f.files}
    ctor = json.loads(str(z["ctor_json"]))
    assert {k: ctor[k] for k in MODEL} == json.loads(json.dumps(MODEL))
    state = _part(z, "sd:")
    x, kw = torch.from_numpy(z["x"]), _part(z, "kw:")
    assert x.shape[1:] == (INPUT_LEN, 1) and x.shape[0] > 100

    # predict_once's steps (predict.py:619-745): build, warm up, size the id table as the checkpoint has it,
    # strict load, eval, remember the id vocabulary of the scaler's ids
    model = ftn.models.TimesNet(**ctor)
    with torch.no_grad():
        model(torch.from_numpy(z["warm_x"]), **_part(z, "warm_kw:"))
    emb = state["series_embedding.weight"]
    if tuple(model.series_embedding.weight.shape) != tuple(emb.shape):
        model.series_embedding = torch.nn.Embedding(*emb.shape, dtype=emb.dtype)
    model.load_state_dict(state, strict=True)
    model.eval()
    model._series_id_vocab = int(model.series_embedding.num_embeddings)
    model._series_id_reference = torch.arange(model._series_id_vocab, dtype=torch.long)
    assert model._series_id_vocab == int(z["id_vocab"])
    assert torch.equal(model._series_id_reference, torch.from_numpy(z["id_reference"]))
    with torch.inference_mode():
        rate, disp = model(x, **kw)

    assert all(b._period_calls > 0 for b in model.blocks)
    np.testing.assert_allclose(rate.numpy(), z["rate"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(disp.numpy(), z["disp"], rtol=1e-5, atol=1e-6)
    # the submission's numbers: one column per series, PRED_LEN rows, clipped at zero ("none" normalisation)
    want = z["submission"]
    assert want.shape == (PRED_LEN, x.shape[0]) and len(z["submission_row_key"]) == PRED_LEN
    a = np.clip(rate.numpy()[:, :PRED_LEN, 0].T.astype(np.float64), 0.0, None)
    assert np.isfinite(a).all() and (a >= 0).all() and a.max() > 0
    np.testing.assert_allclose(a, want, rtol=1e-5, atol=1e-6)
