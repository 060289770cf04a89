"""Scoring on the host side (no GPU): the exports, the torch backend of ``score.negative_binomial_nll`` /
``negative_binomial_mask`` against what the reference returned (tests/golden/score_*.npz, written by
make_golden_score.py), ``ForecastScorer`` on the CPU and ``eval_metrics`` against the reference's ``_eval_metrics``,
``wsmape_grouped``, the form rule of ``ftn_score_columns`` over a table, and every argument error before a launch."""
import itertools

import numpy as np
import pytest
import torch

from conftest import GOLDEN

U = 2.0 ** -24
NLL_CASES = ("full", "none", "float", "bh", "b")
EVAL_CASES = ("shared", "pipeline", "nomask")


def _load(name):
    with np.load(GOLDEN / f"{name}.npz") as z:
        return {k: z[k] for k in z.files}


def test_abi_version_and_exports(ftn):
    assert {"ftn_score_columns", "ftn_score_fold", "ftn_score_form"} <= set(ftn.lib.EXPORTS)
    lib = ftn.lib.load()
    assert lib.ftn_abi_version() == 14 and ftn.lib.ABI_VERSION == 14
    assert ftn.lib.SCORE_PART_BYTES == 24


def test_package_exports_score(ftn):
    sc = ftn.score
    for name in ("negative_binomial_mask", "negative_binomial_nll", "ForecastScorer", "eval_metrics"):
        assert callable(getattr(sc, name)), name


@pytest.mark.parametrize("case", NLL_CASES)
def test_torch_backend_is_the_references_function(case, ftn):
    """The same ops on the same CPU: rtol 1e-6 covers a different thread count in torch's sum."""
    sc = ftn.score
    z = _load(f"score_nll_{case}")
    y, rate, disp = (torch.from_numpy(z[k]) for k in ("y", "rate", "disp"))
    mask = torch.from_numpy(z["mask"]) if "mask" in z else None
    got = sc.negative_binomial_nll(y, rate, disp, mask)
    assert sc._last_backend == "torch" and got.dim() == 0 and got.dtype == torch.float32
    np.testing.assert_allclose(float(got), float(z["nll"]), rtol=1e-6)
    valid = sc.negative_binomial_mask(y, rate, disp, mask)
    assert valid.dtype == torch.bool and np.array_equal(valid.numpy(), z["valid"])


def test_torch_backend_reproduces_the_nan_poisoning(ftn):
    """A masked-out NaN makes the reference's mean NaN (ll * 0): the torch backend is the reference's function."""
    sc = ftn.score
    z = _load("score_nll_full")
    y, rate, disp = (torch.from_numpy(z[k]).clone() for k in ("y", "rate", "disp"))
    mask = torch.from_numpy(z["mask"]).clone()
    mask[1, 2, 3] = False
    assert bool(torch.isfinite(sc.negative_binomial_nll(y, rate, disp, mask)))
    rate[1, 2, 3] = float("nan")
    assert bool(torch.isnan(sc.negative_binomial_nll(y, rate, disp, mask)))


def _batches(z):
    out = []
    for i in range(3):
        b = {k.split(":")[1]: torch.from_numpy(v) for k, v in z.items() if k.startswith(f"b{i}:")}
        out.append(b)
    return out


class Recorded(torch.nn.Module):
    """Returns the recorded (rate, dispersion) of its calls in turn."""

    def __init__(self, outs):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.outs, self.i = outs, 0

    def forward(self, xb, **kw):
        self.i += 1
        return self.outs[self.i - 1]


@pytest.mark.parametrize("case", EVAL_CASES)
def test_scorer_on_the_cpu_reproduces_eval_metrics(case, ftn):
    """nll at rtol 1e-6; smape at atol 8 u: each term is <= 2 and passes through four fp32 roundings."""
    sc = ftn.score
    z = _load(f"score_eval_{case}")
    names = [str(s) for s in z["names"]]
    use_mask = bool(z["use_loss_mask"])
    scorer = sc.ForecastScorer(len(names), "cpu")
    tuples, outs = [], []
    for b in _batches(z):
        mask = (b["mask"] > 0) if use_mask else None
        scorer.update(b["y"], b["rate"], b["disp"], mask, b.get("ids"))
        tuples.append((b["x"], b["y"], b["mask"]) if "ids" not in b else
                      (b["x"], b["y"], b["mask"], None, None, None, b["ids"]))
        outs.append((b["rate"], b["disp"]))
    assert scorer._last_backend == "torch"
    res = scorer.result()
    np.testing.assert_allclose(res["nll"], float(z["nll"]), rtol=1e-6)
    assert abs(res["smape"] - float(z["smape"])) <= 8 * U
    assert res["nll_count"].sum() == sum(int(((b["mask"] > 0) if use_mask else torch.ones_like(b["y"])).sum())
                                         for b in _batches(z))
    via = sc.eval_metrics(Recorded(outs), tuples, "direct", outs[0][0].shape[1], use_loss_mask=use_mask,
                          n_series=len(names))
    assert via["nll"] == res["nll"] and via["smape"] == res["smape"]
    assert np.array_equal(via["nll_sum"], res["nll_sum"]) and np.array_equal(via["smape_count"], res["smape_count"])
    # wsmape_grouped: per-item means of fp32 terms, store means, weights - a handful of roundings of values <= 2
    assert abs(scorer.wsmape_grouped(names) - float(z["wsmape"])) <= 8 * U
    assert abs(float(z["wsmape_check"]) - float(z["wsmape"])) <= 8 * U
    weights = {str(k): float(v) for k, v in zip(z["weight_names"], z["weight_values"])}
    assert abs(scorer.wsmape_grouped(names, weights) - float(z["wsmape_weighted"])) <= 8 * U


def test_scorer_cpu_order_and_edges(ftn):
    sc = ftn.score
    z = _load("score_eval_shared")
    bs = _batches(z)
    one, two = sc.ForecastScorer(5, "cpu"), sc.ForecastScorer(5, "cpu")
    for b in bs[:2]:
        one.update(b["y"], b["rate"], b["disp"], b["mask"] > 0)
    cat = {k: torch.cat([bs[0][k], bs[1][k]]) for k in ("y", "rate", "disp", "mask")}
    two.update(cat["y"], cat["rate"], cat["disp"], cat["mask"] > 0)
    r1, r2 = one.result(), two.result()
    assert all(np.array_equal(r1[k], r2[k]) for k in ("nll_sum", "smape_sum", "nll_count", "smape_count"))
    b = bs[0]
    empty = sc.ForecastScorer(5, "cpu")
    empty.update(b["y"], b["rate"], b["disp"], torch.zeros_like(b["y"], dtype=torch.bool))
    r = empty.result()
    assert r["nll"] == 0.0 and r["smape"] == 0.0 and r["nll_count"].sum() == 0
    bad = sc.ForecastScorer(5, "cpu")
    bad.update(b["y"], b["rate"], b["disp"], None, torch.tensor([0, 1, 2, 3, 5]))
    with pytest.raises(ValueError, match="outside"):
        bad.result()
    with pytest.raises(ValueError, match="slots"):
        sc.ForecastScorer(4, "cpu").update(b["y"], b["rate"], b["disp"])
    one.reset()
    assert one.result()["nll_count"].sum() == 0


# ------------------------------------------------------------------------------------------------------ the form rule
def form_rule(H, N, strides, mis):
    """``score_form`` (csrc/score.hip) restated: four columns per lane with 16-byte loads when N, every batch stride
    and every address allow them; H in segments of max(4, ceil(H / 8)) rows."""
    seg = max(4, -(-H // 8))
    vec = N % 4 == 0 and all(s % 4 == 0 for s in strides) and mis == 0
    return f"k_score_cols<{4 if vec else 1}>", -(-H // seg), seg


TABLE = list(itertools.product((1, 4, 5, 7, 24, 32, 33, 96, 97, 720), (1, 4, 5, 8, 37, 64, 512),
                               ((0, 0, 0), (4096, 4096, 4096), (4097, 4096, 4096), (4096, 4098, 4096), (64, 64, 65)),
                               (0, 4, 8, 12)))


def test_form_rule_over_the_table(ftn):
    seen = set()
    for H, N, strides, mis in TABLE:
        got = ftn.runtime.score_form_of(H, N, strides, mis)
        assert got == form_rule(H, N, strides, mis), (H, N, strides, mis, got)
        seen.add((got[0], got[1]))
    assert {f for f, _ in seen} == {"k_score_cols<4>", "k_score_cols<1>"}
    assert {n for _, n in seen} == {1, 2, 6, 7, 8}
    lib = ftn.lib.load()
    assert lib.ftn_score_form(96, 512, 0, 0, 0, 0) == 2 | 8 << 4 | 12 << 8
    assert lib.ftn_score_form(7, 5, 0, 0, 0, 0) == 2 << 4 | 4 << 8


@pytest.mark.parametrize("args", [(0, 4, 0, 0, 0, 0), (4, 0, 0, 0, 0, 0), (4, 4, -4, 0, 0, 0), (4, 4, 0, 0, 0, 2),
                                  (4, 4, 0, 0, 0, 16), (1 << 16, 1 << 16, 0, 0, 0, 0)])
def test_form_rejects_bad_arguments(args, ftn):
    lib = ftn.lib.load()
    assert lib.ftn_score_form(*args) < 0
    assert b"ftn_score_form" in lib.ftn_last_error()


A, M = 0x10000, 0x10004          # stand-ins for device addresses: 16-byte aligned / 4 bytes past a boundary
GOOD = dict(y=A, ybs=64, rate=A, rbs=64, disp=A, dbs=64, mask=None, kind=0, eps=1e-8, B=2, H=8, N=8, part=A, ll=None)
BAD = {
    "null y": dict(y=None), "null rate": dict(rate=None), "null dispersion": dict(disp=None),
    "null part": dict(part=None), "B = 0": dict(B=0), "H = 0": dict(H=0), "N < 0": dict(N=-1),
    "y batch stride below H N": dict(ybs=63), "rate batch stride below H N": dict(rbs=8),
    "H N beyond int32": dict(H=1 << 16, N=1 << 16, B=1), "B N beyond int32": dict(B=1 << 16, N=1 << 16, H=1),
    "mask without a kind": dict(mask=A), "kind without a mask": dict(kind=1), "unknown mask kind": dict(mask=A, kind=3),
    "eps = 0": dict(eps=0.0), "y off by 2": dict(y=A + 2), "part off by 4": dict(part=M),
}


@pytest.mark.parametrize("name", list(BAD))
def test_columns_reject_bad_arguments_before_any_launch(name, ftn):
    lib = ftn.lib.load()
    a = {**GOOD, **BAD[name]}
    assert lib.ftn_score_form(8, 8, 0, 0, 0, 0) > 0                     # leaves an earlier message out of the way
    rc = lib.ftn_score_columns(a["y"], a["ybs"], a["rate"], a["rbs"], a["disp"], a["dbs"], a["mask"], a["kind"],
                               a["eps"], a["B"], a["H"], a["N"], a["part"], a["ll"], None)
    assert rc < 0
    assert lib.ftn_last_error().decode().startswith("ftn_score_columns")
    with pytest.raises(ValueError, match="ftn_score_columns"):
        ftn.lib.check(rc, "ftn_score_columns")


FOLD_GOOD = dict(part=A, B=2, N=8, kind=0, ids=None, order=None, seg=None, acc=A, slots=8, err=A)
FOLD_BAD = {
    "null part": dict(part=None), "null acc": dict(acc=None), "null err": dict(err=None), "n_slots = 0": dict(slots=0),
    "n_slots < 0": dict(slots=-2), "B = 0": dict(B=0), "B N beyond int32": dict(B=1 << 16, N=1 << 16),
    "more series than slots": dict(slots=7), "ids without a kind": dict(ids=A), "kind 1 without ids": dict(kind=1),
    "kind 2 without order": dict(kind=2, seg=A), "kind 2 without seg_start": dict(kind=2, order=A),
    "unknown kind": dict(kind=3), "acc off by 4": dict(acc=M),
}


@pytest.mark.parametrize("name", list(FOLD_BAD))
def test_fold_rejects_bad_arguments_before_any_launch(name, ftn):
    lib = ftn.lib.load()
    a = {**FOLD_GOOD, **FOLD_BAD[name]}
    assert lib.ftn_score_form(8, 8, 0, 0, 0, 0) > 0
    rc = lib.ftn_score_fold(a["part"], a["B"], a["N"], a["kind"], a["ids"], a["order"], a["seg"], a["acc"],
                            a["slots"], a["err"], None)
    assert rc < 0
    assert lib.ftn_last_error().decode().startswith("ftn_score_fold")


def test_wrappers_validate_layout_on_the_host(ftn):
    rt = ftn.runtime
    y, r, d = torch.zeros(2, 8, 8), torch.ones(2, 8, 8), torch.ones(2, 8, 8)
    with pytest.raises(ValueError, match="y must be an fp32 device tensor"):
        rt.score_columns(y, r, d)
    with pytest.raises(ValueError, match="\\[B, H, N\\]"):
        rt.score_columns(y[0], r, d)
    with pytest.raises(ValueError, match="rate has shape"):
        rt.score_columns(y, r[:, :7], d)
    with pytest.raises(ValueError, match="y must be an fp32"):
        rt.score_columns(y.double(), r, d)
    with pytest.raises(ValueError, match="y needs contiguous rows"):
        rt.score_columns(torch.zeros(2, 8, 16)[:, :, ::2], r, d)
    with pytest.raises(ValueError, match="dispersion needs contiguous rows"):
        rt.score_columns(y, r, torch.ones(2, 16, 8)[:, ::2])
    part = torch.zeros(16 * 24, dtype=torch.uint8)
    with pytest.raises(ValueError, match="part must be contiguous uint8 device"):
        rt.score_fold(part, 2, 8, part, torch.zeros(1, dtype=torch.int32))
