"""The NB sampler on the MI355X (``ftn_nb_sample`` behind ``score.nb_sample``) and the sampled recursive forecast
(``forecast.forecast_sample_paths``): the uniforms bit for bit against the numpy mirror of the contract
(tests/nbs_checks.py), the samples against the scipy fixtures of tests/golden/make_golden_sample.py under the tie rule
and against the torch backend, and the device forecast bit for bit against ``forecast_sample_paths_loop``."""
import ctypes as C

import numpy as np
import pytest
import torch

import nbs_checks as ns
from test_gpu_recursive import _inputs, _model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a ROCm device"
    return torch.device("cuda:0")


def _fix(name, dev):
    z = ns.load(name)
    rate, disp = (torch.from_numpy(np.array(z[k])).to(dev) for k in ("rate", "disp"))
    return z, rate, disp, int(z["S"]), int(z["seed"]), int(z["offset"])


@pytest.fixture(scope="module")
def ran(ftn, dev):
    """Every fixture through the kernel, once: name -> (samples, uniforms, flag) on the host."""
    out = {}
    for name in ns.FIXTURES:
        z, rate, disp, S, seed, off = _fix(name, dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        x, u = ftn.score.nb_sample(rate, disp, S, seed, off, return_uniforms=True, flag=flag)
        assert ftn.score._last_backend == "hip"
        out[name] = (x.cpu(), u.cpu(), int(flag))
    return out


def _views(t, dev):
    """``t`` [B,H,N] as a batch-strided view (stride not a multiple of 4), a 4-byte-misaligned view, and a
    batch-strided view that keeps the vector form."""
    B, H, N = t.shape
    wide = torch.zeros(B, H * N + 2, device=dev)
    wide[:, :H * N] = t.reshape(B, -1)
    buf = torch.zeros(B * H * N + 1, device=dev)
    buf[1:] = t.reshape(-1)
    wide4 = torch.zeros(B, H * N + 4, device=dev)
    wide4[:, :H * N] = t.reshape(B, -1)
    strided, offset, v4 = wide[:, :H * N].view(B, H, N), buf[1:].view(B, H, N), wide4[:, :H * N].view(B, H, N)
    assert strided.stride(0) == H * N + 2 and offset.data_ptr() % 16 == 4 and v4.stride(0) == H * N + 4
    return strided, offset, v4


@pytest.mark.parametrize("S", [1, 3, 4, 5, 9])
def test_uniforms_are_the_contract_in_both_forms(S, ftn, dev):
    rt = ftn.runtime
    seed = (0xC0FFEE11 << 32) | 0x0BADF00D
    for shape, form in (((4, 24, 36), "vec4"), ((3, 7, 5), "scalar"), ((1, 5, 8), "vec4"), ((1, 3, 7), "scalar"),
                        ((2, 130, 8), "vec4")):
        rate = torch.rand(shape, device=dev) * 3.0 + 0.1
        disp = torch.rand(shape, device=dev) + 0.1
        assert rt.nb_sample_form(rate, disp) == form
        for off in (0, 5):
            x, flag, u = rt.nb_sample(rate, disp, S, seed, off, want_uniforms=True)
            assert int(flag) == 0 and u.dtype == torch.float64
            assert np.array_equal(u.cpu().numpy(), ns.uniforms_numpy(S, shape, seed, off)), (shape, off)
        if shape[0] > 1 and form == "vec4":
            for rv, form_v in zip(_views(rate, dev), ("scalar", "scalar", "vec4")):
                assert rt.nb_sample_form(rv, disp) == form_v
                xv, _, uv = rt.nb_sample(rv, disp, S, seed, 5, want_uniforms=True)
                assert torch.equal(uv, u) and torch.equal(xv, x), form_v
            dv = _views(disp, dev)[0]
            xv, _, uv = rt.nb_sample(rate, dv, S, seed, 5, want_uniforms=True)
            assert rt.nb_sample_form(rate, dv) == "scalar" and torch.equal(uv, u) and torch.equal(xv, x)


@pytest.mark.parametrize("name", ns.FIXTURES)
def test_fixtures_under_the_tie_rule(name, ran):
    z = ns.load(name)
    x, u, flag = ran[name]
    assert x.dtype == torch.float32 and flag == 0
    assert np.array_equal(u.numpy(), ns.uniforms_numpy(int(z["S"]), z["rate"].shape, int(z["seed"]), int(z["offset"])))
    ties = ns.check_samples(x.numpy(), z, name)
    print(f"NBS_TIES hip {name} {ties}/{z['k_star'].size} kmax={float(x.max()):.0f}")


def test_forms_agree_on_the_vector_fixture(ftn, dev, ran):
    z, rate, disp, S, seed, off = _fix("std_vector", dev)
    assert ftn.runtime.nb_sample_form(rate, disp) == "vec4"
    for view, form in zip(_views(rate, dev), ("scalar", "scalar", "vec4")):
        assert ftn.runtime.nb_sample_form(view, disp) == form
        x, flag, _ = ftn.runtime.nb_sample(view, disp, S, seed, off)
        assert int(flag) == 0 and torch.equal(x.cpu(), ran["std_vector"][0]), form


@pytest.mark.parametrize("name", ["std_vector", "std_scalar"])
def test_hip_equals_torch_outside_near_ties(name, ftn, dev, ran):
    z, rate, disp, S, seed, off = _fix(name, dev)
    want = ftn.score.nb_sample(rate.cpu(), disp.cpu(), S, seed, off)
    assert ftn.score._last_backend == "torch"
    got = ran[name][0]
    differ = (got != want).numpy()
    print(f"NBS_BACKENDS {name} differ at {int(differ.sum())} draws, {int((differ & ~z['tie']).sum())} outside ties")
    assert not bool((differ & ~z["tie"]).any())
    if name == "std_scalar":                                # the torch backend on device tensors (launch-bound: once)
        on_dev = ftn.score.nb_sample(rate, disp, S, seed, off, backend="torch")
        assert ftn.score._last_backend == "torch" and not bool(((on_dev.cpu() != got).numpy() & ~z["tie"]).any())


def test_seed_by_device_word_and_replays(ftn, dev, ran):
    z, rate, disp, S, seed, off = _fix("std_scalar", dev)
    for word in (torch.tensor([seed - (1 << 64)], dtype=torch.int64, device=dev),
                 torch.tensor([seed - (1 << 64)], dtype=torch.int64, device=dev).view(torch.uint64)):
        x = ftn.score.nb_sample(rate, disp, S, word, off)
        assert ftn.score._last_backend == "hip" and torch.equal(x.cpu(), ran["std_scalar"][0])
    again = ftn.score.nb_sample(rate, disp, S, seed, off)
    assert torch.equal(again.cpu(), ran["std_scalar"][0])
    other = ftn.score.nb_sample(rate, disp, S, seed + 1, off)
    assert not torch.equal(other.cpu(), ran["std_scalar"][0])
    S1 = ftn.score.nb_sample(rate, disp, 3, seed, off)
    assert torch.equal(S1.cpu(), ran["std_scalar"][0][:3])


def test_invalid_and_out_of_range(ftn, dev):
    sc = ftn.score
    z, rate, disp, S, seed, off = _fix("std_vector", dev)
    base = sc.nb_sample(rate, disp, 3, 11)
    r2, d2 = rate.clone(), disp.clone()
    bad = torch.zeros(rate.shape, dtype=torch.bool, device=dev)
    r2[0, 1, 2], d2[1, 3, 4], r2[2, 5, 6], d2[3, 7, 9] = float("nan"), float("inf"), float("inf"), float("nan")
    bad[0, 1, 2] = bad[1, 3, 4] = bad[2, 5, 6] = bad[3, 7, 9] = True
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    x = sc.nb_sample(r2, d2, 3, 11, flag=flag)
    assert int(flag) == 0 and bool(torch.isnan(x[:, bad]).all()) and torch.equal(x[:, ~bad], base[:, ~bad])
    r3 = rate.clone()
    r3[1, 1, 1] = 1e8
    x = sc.nb_sample(r3, disp, 3, 11, flag=flag)
    assert int(flag) == ftn.lib.FTN_NBQ_RANGE == 2
    assert bool(torch.isnan(x[:, 1, 1, 1]).all()) and int(torch.isnan(x).sum()) == 3
    small, eps = torch.full_like(rate, 1e-12), torch.full_like(rate, 1e-8)          # below eps = eps
    assert torch.equal(sc.nb_sample(small, disp, 2, 5), sc.nb_sample(eps, disp, 2, 5))


def test_c_entry_rejects_bad_arguments(ftn, dev):
    lib = ftn.lib.load()
    rate = torch.ones(2, 3, 4, device=dev)
    out = torch.empty(4, 2, 3, 4, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream

    def call(S=2, r=rate.data_ptr(), rs=12, ds=12, o=out.data_ptr(), f=flag.data_ptr(), H=3, eps=1e-8):
        return lib.ftn_nb_sample(r, rs, rate.data_ptr(), ds, 2, H, 4, S, 7, None, 0, eps, o, None, f, st)

    assert call() == 0
    assert call(S=-1) < 0 and call(S=0) < 0
    assert call(f=None) < 0 and call(r=None) < 0 and call(o=None) < 0
    assert call(rs=-12) < 0 and call(ds=8) < 0 and call(rs=11) < 0
    assert call(H=0) < 0 and call(eps=0.0) < 0
    assert b"ftn_nb_sample" in lib.ftn_last_error()
    assert lib.ftn_nb_sample_form(0, 0, 0, 0) < 0 and lib.ftn_nb_sample_form(4, 0, 0, 2) < 0
    with pytest.raises(ValueError):
        ftn.runtime.nb_sample(rate, rate, 2, seed=torch.zeros(1, dtype=torch.int64))    # a seed word on the host
    with pytest.raises(ValueError):
        ftn.runtime.nb_sample(rate, rate, 2, out=torch.empty(2, 2, 3, 5, device=dev))
    torch.cuda.synchronize()
    assert int(flag) == 0


# ------------------------------------------------------------------------------------------ sampled recursive forecasts
SHAPES = [(64, 32, 24, 29, 1, 12, 0, "decoupled", 3), (128, 40, 24, 24, 2, 8, 3, "decoupled", 2)]


@pytest.mark.parametrize("d_model,N,L,T,B,H,marks,norm,P", SHAPES)
def test_sample_paths_equal_the_loop(d_model, N, L, T, B, H, marks, norm, P, ftn, dev):
    fc = ftn.forecast
    model = _model(ftn, dev, d_model, N, L, marks, norm)
    x, kw = _inputs(dev, B, T, N, H, marks, seed=3)
    with torch.inference_mode():
        want = fc.forecast_sample_paths_loop(model, x, H, P, seed=17, **kw)
        want_periods = model.period_selector.last_selected_periods.tolist()
        model._last_embed_backend = None
        ftn.score._last_backend = None
        got = fc.forecast_sample_paths(model, x, H, P, seed=17, **kw)
        periods = model.period_selector.last_selected_periods.tolist()
        other = fc.forecast_sample_paths(model, x, H, P, seed=18, **kw)
    assert model._last_embed_backend == "hip" and model._last_head_backend == "hip"
    assert all(b._last_backend == "hip" for b in model.blocks) and ftn.score._last_backend == "hip"
    for g, w in zip(got, want):
        assert tuple(g.shape) == (P, B, H, N) and torch.equal(g, w)
    assert periods == want_periods
    assert bool(torch.isfinite(got[0]).all()) and bool((got[0] == got[0].round()).all())
    assert not torch.equal(other[0][:, :, 0], got[0][:, :, 0])                  # the samples change from step 0,
    assert torch.equal(other[1][:, :, 0], got[1][:, :, 0])                      # the rates from step 1
    assert not torch.equal(other[1][:, :, 1], got[1][:, :, 1])


def test_overflowing_rates_raise_with_their_step(ftn, dev):
    fc = ftn.forecast
    d_model, N, L, T, B, H, marks, norm, P = SHAPES[0]
    model = _model(ftn, dev, d_model, N, L, marks, norm)
    x, kw = _inputs(dev, B, T, N, H, marks, seed=3)
    with torch.inference_mode():
        rate0, _ = fc.forecast_recursive_batch(model, x, 1, **kw)
        assert float(rate0.max()) < 1e6
        for run in (fc.forecast_sample_paths, fc.forecast_sample_paths_loop):
            with pytest.raises(RuntimeError, match="step 0"):
                run(model, x * 1e9, 3, P, seed=1, **kw)
        s, r, d = fc.forecast_sample_paths(model, x, 2, P, seed=1, **kw)         # and the model is usable afterwards
    assert bool(torch.isfinite(s).all())
