"""The ``torch`` backend of ``score.nb_cdf`` / ``nb_quantiles`` / ``prediction_interval`` / ``interval_metrics`` on
CPU tensors against the scipy fixtures (tests/golden/make_golden_quantile.py), under the rules of the device tests:
the CDF within 1e-6 of min(F, 1 - F) (the bound the quantile rule assumes; through fp64, before the fp32 rounding),
quantiles exact outside near ties, and the argument errors."""
import numpy as np
import pytest
import torch

import nbq_checks as nq


def _t(z, *names):
    return [torch.from_numpy(np.array(z[n])) for n in names]


@pytest.mark.parametrize("name", nq.FIXTURES)
def test_torch_backend_against_the_fixtures(name, ftn):
    sc = ftn.score
    z = nq.load(name)
    y, rate, disp = _t(z, "y", "rate", "disp")
    F64, flag = sc._nb_cdf_torch(y, rate, disp, 1e-8)
    e = nq.cdf_error(F64.numpy(), z["F_y"])
    print(f"NBQ_CDF_ERR torch {name} {e:.3e}")
    assert e <= 1e-6 and int(flag) == 0
    F = sc.nb_cdf(y, rate, disp)
    assert sc._last_backend == "torch" and F.dtype == torch.float32 and torch.equal(F, F64.float())
    Q = sc.nb_quantiles(rate, disp, list(z["levels"]), check=True)
    assert sc._last_backend == "torch" and Q.dtype == torch.float32 and tuple(Q.shape) == z["k_star"].shape
    nq.check_quantiles(Q.numpy(), z, name)
    assert bool((Q[1:] >= Q[:-1]).all())
    lo, hi = sc.prediction_interval(rate, disp, 0.95)
    assert torch.equal(lo, Q[list(z["levels"]).index(0.025)]) and torch.equal(hi, Q[list(z["levels"]).index(0.975)])


def test_levels_in_any_order_and_more_than_eight(ftn):
    sc = ftn.score
    z = nq.load("scalar")
    rate, disp = _t(z, "rate", "disp")
    levels = [0.9, 0.025, 0.5, 0.975, 0.1, 0.3, 0.7, 0.05, 0.95]
    Q = sc.nb_quantiles(rate, disp, levels)
    ref = sc.nb_quantiles(rate, disp, sorted(levels))
    for i, q in enumerate(levels):
        assert torch.equal(Q[i], ref[sorted(levels).index(q)]), q
    for q, row in zip(z["levels"], z["k_star"]):
        assert np.array_equal(Q[levels.index(float(q))].numpy().astype(np.float64), row)


def test_edges_on_the_torch_backend(ftn):
    sc = ftn.score
    z = nq.load("scalar")
    y, rate, disp = _t(z, "y", "rate", "disp")
    base = sc.nb_quantiles(rate, disp, [0.1, 0.9])
    r2, d2 = rate.clone(), disp.clone()
    r2[0, 1, 2], d2[1, 3, 4], r2[2, 5, 1] = float("nan"), float("inf"), float("inf")
    Q = sc.nb_quantiles(r2, d2, [0.1, 0.9], check=True)            # invalid elements do not raise the flag
    bad = torch.zeros(rate.shape, dtype=torch.bool)
    bad[0, 1, 2] = bad[1, 3, 4] = bad[2, 5, 1] = True
    assert bool(torch.isnan(Q[:, bad]).all()) and torch.equal(Q[:, ~bad], base[:, ~bad])
    F = sc.nb_cdf(y, r2, d2)
    assert bool(torch.isnan(F[bad]).all()) and torch.equal(F[~bad], sc.nb_cdf(y, rate, disp)[~bad])
    # below eps = eps; y < 0 = 0; fractional y = floor(y)
    small = torch.full_like(rate, 1e-12)
    eps = torch.full_like(rate, 1e-8)
    assert torch.equal(sc.nb_quantiles(small, disp, [0.5]), sc.nb_quantiles(eps, disp, [0.5]))
    assert torch.equal(sc.nb_cdf(y, rate, small), sc.nb_cdf(y, rate, eps))
    assert torch.equal(sc.nb_cdf(torch.full_like(y, -2.0), rate, disp), sc.nb_cdf(torch.zeros_like(y), rate, disp))
    yy = torch.floor(y.clamp(min=0.0))
    assert torch.equal(sc.nb_cdf(yy + 0.5, rate, disp), sc.nb_cdf(yy, rate, disp))
    # an answer beyond 2^24: NaN there alone, and check=True raises
    r3 = rate.clone()
    r3[1, 1, 1] = 1e8
    Q = sc.nb_quantiles(r3, disp, [0.5])
    assert bool(torch.isnan(Q[0, 1, 1, 1])) and int(torch.isnan(Q).sum()) == 1
    with pytest.raises(ValueError, match="2\\^24"):
        sc.nb_quantiles(r3, disp, [0.5], check=True)


def test_argument_errors(ftn):
    sc = ftn.score
    rate, disp = torch.ones(2, 3, 4), torch.ones(2, 3, 4)
    for bad in ([0.0], [1.0], [0.5, 1.5], [-0.1], []):
        with pytest.raises(ValueError):
            sc.nb_quantiles(rate, disp, bad)
    with pytest.raises(ValueError):
        sc.prediction_interval(rate, disp, 1.0)
    with pytest.raises(ValueError):
        sc.nb_quantiles(rate, torch.ones(2, 3, 5), [0.5])
    with pytest.raises(ValueError):
        sc.nb_cdf(torch.ones(2, 3, 5), rate, disp)
    assert {"ftn_nb_cdf", "ftn_nb_quantiles", "ftn_nbq_form"} <= set(ftn.lib.EXPORTS)
    assert ftn.lib.FTN_QMAX == sc.NBQ_QMAX == 8 and ftn.lib.FTN_NBQ_RANGE == sc.NBQ_FLAG_RANGE == 2


def test_interval_metrics_against_numpy(ftn):
    """Coverage is a ratio of counts below 2^24 (exact in fp32 up to the one division); pinball and PIT are fp32
    means of n terms: |error| <= (n + 2) 2^-24 times the mean magnitude, asserted as n 2^-23."""
    sc = ftn.score
    z = nq.load("vector")
    y, rate, disp = _t(z, "y", "rate", "disp")
    mask = torch.rand(y.shape, generator=torch.Generator().manual_seed(0)) >= 0.2
    for m in (None, mask):
        got = sc.interval_metrics(y, rate, disp, list(z["levels"]), m)
        valid = np.isfinite(z["y"]) & (np.ones(y.shape, bool) if m is None else m.numpy())
        cov, pin, pit = nq.interval_metrics_numpy(z, valid)
        n = int(valid.sum())
        assert int(got["count"]) == n
        ties = int(((np.abs(z["F_k"] - z["levels"].reshape(-1, 1, 1, 1)) <= nq.band(z["levels"])) |
                    (np.abs(z["F_km1"] - z["levels"].reshape(-1, 1, 1, 1)) <= nq.band(z["levels"]))).sum())
        assert np.all(np.abs(got["coverage"].numpy() - cov) <= ties / n + 2 * nq.U32)
        tol = n * 2.0 ** -23
        assert np.all(np.abs(got["pinball"].numpy() - pin) <= tol * np.maximum(pin, 1.0) + ties / n)
        assert abs(float(got["pit_mean"]) - pit) <= tol


def _same_bits(got, want):
    return got.dtype == want.dtype == np.float32 and got.shape == want.shape and \
        np.array_equal(got.view(np.int32), want.view(np.int32))


def test_one_search_reproduces_the_two_it_replaced(ftn):
    """``nb_quantiles`` and ``nb_sample`` on the torch backend against tests/golden/nb_torch_parent.npz, the outputs of
    the two search loops that ``nbdist._nb_search`` replaced (tests/golden/make_golden_nb_torch.py): every fp32 word,
    NaN positions included, and the flags."""
    import nbs_checks as ns

    sc = ftn.score
    with np.load(nq.GOLDEN / "nb_torch_parent.npz") as z:
        pin = {k: z[k] for k in z.files}
    edge = (torch.from_numpy(pin["edge_rate"]), torch.from_numpy(pin["edge_disp"]))
    q_cases = [(n, *_t(nq.load(n), "rate", "disp"), list(nq.load(n)["levels"]))
               for n in ("scalar", "pipeline", "large", "tiny")]
    q_cases.append(("edge", *edge, [0.025, 0.5, 0.975]))
    for name, rate, disp, levels in q_cases:
        out = sc.nb_quantiles(rate, disp, levels)
        assert sc._last_backend == "torch" and _same_bits(out.numpy(), pin[f"q_{name}"]), name
        out2, flag = sc._nb_quantiles_torch(rate, disp, [float(q) for q in levels], 1e-8)
        assert torch.equal(out2.view(torch.int32), out.view(torch.int32)), name
        assert int(flag) == int(pin[f"qflag_{name}"]), name
    s_cases = [(n, *_t(ns.load(n), "rate", "disp"), *(int(ns.load(n)[k]) for k in ("S", "seed", "offset")))
               for n in ("std_scalar", "tiny", "large")]
    s_cases.append(("edge", *edge, 5, 11, 2))
    for name, rate, disp, S, seed, offset in s_cases:
        flag = torch.zeros(1, dtype=torch.int32)
        out = sc.nb_sample(rate, disp, S, seed, offset, backend="torch", flag=flag)
        assert sc._last_backend == "torch" and _same_bits(out.numpy(), pin[f"s_{name}"]), name
        assert int(flag) == int(pin[f"sflag_{name}"]), name
    assert int(pin["qflag_edge"]) == int(pin["sflag_edge"]) == sc.NBQ_FLAG_RANGE       # the pin holds a raised flag too
    assert np.isnan(pin["q_edge"]).any() and np.isnan(pin["s_edge"]).any()
