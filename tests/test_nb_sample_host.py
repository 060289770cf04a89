"""The sampler without a GPU: the Philox generator and the uniforms' contract, the torch backend of ``score.nb_sample``
against the scipy fixtures of tests/golden/make_golden_sample.py, ``path_quantiles`` against numpy, and the semantics
of ``forecast.forecast_sample_paths_loop`` on a small CPU model."""
import numpy as np
import pytest
import torch

import nbs_checks as ns


@pytest.fixture(scope="module")
def ran(ftn):
    """Every fixture through the torch backend, once: name -> (samples, uniforms) on the host."""
    out = {}
    for name in ns.FIXTURES:
        z = ns.load(name)
        rate, disp = torch.from_numpy(np.array(z["rate"])), torch.from_numpy(np.array(z["disp"]))
        x, u = ftn.score.nb_sample(rate, disp, int(z["S"]), int(z["seed"]), int(z["offset"]), return_uniforms=True)
        assert ftn.score._last_backend == "torch"
        out[name] = (x, u)
    return out


def test_philox_known_answers(ftn):
    kat = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
            "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for ctr, key, want in kat:
        assert " ".join(f"{int(w):08x}" for w in ftn.score.philox4x32(ctr, key)) == want
        got = ftn.score.philox4x32([torch.tensor([c, c]) for c in ctr], key)         # as tensors, broadcast
        assert all(w.tolist() == [int(v, 16)] * 2 for w, v in zip(got, want.split()))
        assert " ".join(f"{int(w):08x}" for w in ns.philox_numpy(*ctr, *key)) == want


def test_uniforms_follow_the_contract(ftn):
    sc = ftn.score
    seed, off = (0xDEADBEEF << 32) | 0x12345678, 7
    for S, shape in ((1, (5,)), (5, (3, 7, 5)), (9, (2, 1, 4))):
        u = sc.sample_uniforms(S, shape, seed, off)
        assert u.dtype == torch.float64 and tuple(u.shape) == (S,) + shape
        assert np.array_equal(u.numpy(), ns.uniforms_numpy(S, shape, seed, off))
        assert float(u.min()) > 0.0 and float(u.max()) < 1.0
    u9, u5 = sc.sample_uniforms(9, (3, 7, 5), seed, off), sc.sample_uniforms(5, (3, 7, 5), seed, off)
    assert torch.equal(u9[:5], u5)
    assert not bool((sc.sample_uniforms(5, (3, 7, 5), seed, off + 1) == u5).any())
    assert not bool((sc.sample_uniforms(5, (3, 7, 5), seed ^ (1 << 40), off) == u5).any())
    assert not bool((sc.sample_uniforms(5, (3, 7, 5), seed ^ 1, off) == u5).any())
    for t in (torch.tensor([seed - (1 << 64)], dtype=torch.int64), torch.tensor(seed - (1 << 64), dtype=torch.int64)):
        assert torch.equal(sc.sample_uniforms(5, (3, 7, 5), t, off), u5)
    with pytest.raises(ValueError):
        sc.sample_uniforms(0, (3,), 0)


@pytest.mark.parametrize("name", ns.FIXTURES)
def test_torch_backend_passes_the_fixtures(name, ran):
    z = ns.load(name)
    x, u = ran[name]
    assert x.dtype == torch.float32
    assert np.array_equal(u.numpy(), ns.uniforms_numpy(int(z["S"]), z["rate"].shape, int(z["seed"]), int(z["offset"])))
    ties = ns.check_samples(x.numpy(), z, name)
    print(f"NBS_TIES torch {name} {ties}/{z['k_star'].size} kmax={float(x.max()):.0f}")


def test_invalid_and_out_of_range(ftn):
    sc = ftn.score
    z = ns.load("std_scalar")
    rate, disp = torch.from_numpy(np.array(z["rate"])), torch.from_numpy(np.array(z["disp"]))
    base = sc.nb_sample(rate, disp, 3, 11)
    r2, d2 = rate.clone(), disp.clone()
    bad = torch.zeros(rate.shape, dtype=torch.bool)
    r2[0, 1, 2], d2[1, 3, 4], r2[2, 5, 1], d2[2, 6, 3] = float("nan"), float("inf"), float("inf"), float("nan")
    bad[0, 1, 2] = bad[1, 3, 4] = bad[2, 5, 1] = bad[2, 6, 3] = True
    flag = torch.zeros(1, dtype=torch.int32)
    x = sc.nb_sample(r2, d2, 3, 11, flag=flag)
    assert int(flag) == 0 and bool(torch.isnan(x[:, bad]).all()) and torch.equal(x[:, ~bad], base[:, ~bad])
    r3 = rate.clone()
    r3[1, 1, 1] = 1e8
    x = sc.nb_sample(r3, disp, 3, 11, flag=flag)
    assert int(flag) == sc.NBQ_FLAG_RANGE == 2
    assert bool(torch.isnan(x[:, 1, 1, 1]).all()) and int(torch.isnan(x).sum()) == 3
    with pytest.raises(ValueError):
        sc.nb_sample(rate, disp, 0)
    with pytest.raises(ValueError):
        sc.nb_sample(rate, disp[:, :, :4], 1)
    with pytest.raises(ValueError, match="hip"):
        sc.nb_sample(rate, disp, 1, backend="hip")


def test_moments_on_a_fixed_seed(ftn):
    """|mean - mu| <= 6 sqrt((mu + alpha mu^2) / n) over n = 4096 draws: six standard errors of the mean.  One fixed
    seed, so the outcome is a constant of the generator and the search, not a random event."""
    cases = [(0.05, 0.5), (1.0, 0.1), (3.0, 2.0), (20.0, 0.3), (150.0, 1.0), (900.0, 0.02)]
    mu = torch.tensor([c[0] for c in cases], dtype=torch.float32).view(1, 1, -1)
    al = torch.tensor([c[1] for c in cases], dtype=torch.float32).view(1, 1, -1)
    n = 4096
    x = ftn.score.nb_sample(mu, al, n, seed=20260101).double()
    mean = x.mean(0).reshape(-1)
    for j, (m, a) in enumerate(cases):
        err, tol = abs(float(mean[j]) - m), 6.0 * ((m + a * m * m) / n) ** 0.5
        print(f"NBS_MOMENT mu={m} alpha={a} mean={float(mean[j]):.4f} err={err:.4f} tol={tol:.4f}")
        assert err <= tol, (m, a, float(mean[j]))


def test_path_quantiles_against_numpy(ftn):
    g = np.random.default_rng(5)
    P, B, H, N = 13, 2, 6, 3
    x = g.poisson(4.0, (P, B, H, N)).astype(np.float32)
    levels = [0.1, 0.5, 0.9, 0.975]
    got = ftn.score.path_quantiles(torch.from_numpy(x), levels)
    assert tuple(got.shape) == (4, B, H, N)
    assert np.array_equal(got.numpy(), np.quantile(x, levels, axis=0, method="inverted_cdf"))
    for w in (2, 3, 6):
        got = ftn.score.path_quantiles(torch.from_numpy(x), levels, window=w)
        sums = x.reshape(P, B, H // w, w, N).sum(3)
        assert tuple(got.shape) == (4, B, H // w, N)
        assert np.array_equal(got.numpy(), np.quantile(sums, levels, axis=0, method="inverted_cdf"))
    with pytest.raises(ValueError, match="window"):
        ftn.score.path_quantiles(torch.from_numpy(x), levels, window=4)
    with pytest.raises(ValueError):
        ftn.score.path_quantiles(torch.from_numpy(x), [1.0])


def _cpu_model(ftn, N, L):
    cfg = dict(input_len=L, pred_len=4, d_model=16, d_ff=32, n_layers=1, k_periods=2, kernel_set=[(3, 3)],
               dropout=0.0, activation="gelu", mode="recursive", use_checkpoint=False)
    torch.manual_seed(0)
    m = ftn.models.TimesNet(**cfg).eval()
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        m(torch.rand(2, L, N, generator=g) + 1.0)
        for p in m.parameters():
            if float(p.abs().sum()) == 0.0:
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
    return m


def test_sample_paths_loop_semantics(ftn):
    fc, sc = ftn.forecast, ftn.score
    N, L, T, B, H, P = 6, 12, 14, 2, 3, 3
    model = _cpu_model(ftn, N, L)
    g = torch.Generator().manual_seed(2)
    x = torch.rand(B, T, N, generator=g) * 4.0 + 1.0
    with torch.no_grad():
        s1, r1, d1 = fc.forecast_sample_paths_loop(model, x, H, P, seed=99)
        s2, r2, d2 = fc.forecast_sample_paths(model, x, H, P, seed=99)              # CPU tensors: the loop
        s3, _, _ = fc.forecast_sample_paths_loop(model, x, H, P, seed=100)
    for t in (s1, r1, d1):
        assert tuple(t.shape) == (P, B, H, N) and t.dtype == torch.float32
    assert torch.equal(s1, s2) and torch.equal(r1, r2) and torch.equal(d1, d2)
    assert not torch.equal(s1, s3)
    for s in range(H):
        want = sc.nb_sample(r1[:, :, s].reshape(P * B, 1, N), d1[:, :, s].reshape(P * B, 1, N), 1, 99, offset=s)[0]
        assert torch.equal(s1[:, :, s].reshape(P * B, 1, N), want)
    with torch.no_grad():
        window = torch.cat([x.repeat(P, 1, 1)[:, 1:], s1[:, :, 0].reshape(P * B, 1, N)], dim=1)
        rate, disp = model(window)
    assert torch.equal(rate.reshape(P, B, N), r1[:, :, 1]) and torch.equal(disp.reshape(P, B, N), d1[:, :, 1])
    assert torch.equal(r1[0, :, 0], r1[P - 1, :, 0])                                 # step 0: every path sees one window
