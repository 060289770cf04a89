"""The RMS norm epilogue of the value embedding on the MI355X (``embed_norm_mode="rms"``: ``ftn_embed_forward_rms``,
``ftn_embed_ring_rms`` and their wide counterparts), from the kernels to the device forecasts:

* the epilogue against ``(v rsqrt(mean v^2 + eps)) gamma + beta`` evaluated in fp64 on the fp64 ``x W^T + add``, at the
  tolerance of the LayerNorm cases of ``test_gpu_shell.py`` / ``test_gpu_shell_wide.py`` (rtol 2e-5, atol 2e-5: the RMS
  norm has one rounding step fewer);
* ring == one pass, bit for bit, on every form and at every d_model - ragged column tiles (36, 100, 132, 260) included,
  which LayerNorm cannot pass on the narrow kernels.  ``forecast._prepare`` has no form list for "rms" because of it;
* row properties: position independence, ``out == beta`` for an all-zero row and for a row whose squares overflow
  fp32, NaN isolation, guard words around the output of all four entry points;
* the reference's ``dropin_rms_recursive`` checkpoint on the device, every shell stage on HIP;
* recursive forecasts, graph replays and sample paths equal to the host loop, with the loop patched out while the
  device path runs;
* the epilogue and ring cases again under ``FTN_EMBED_F32=1``, ``FTN_EMBED_RT=1`` and ``FTN_EMBED_RT=2``, each in a
  fresh child process.
"""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from test_dropin_reference import SHELL_CASES, _fixture, _part
from test_gpu_recursive import _inputs, _loop, _model
from test_gpu_shell import SW_E, _as_window, _window
from test_shell_forms_table import embed_rule
from test_shell_wide_host import embed_wide_rule

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
RTOL, ATOL = 1e-4, 2e-5                      # the project's GPU parity tolerance (model level)
NARROW, WIDE = (4, 36, 64, 100, 128), (132, 256, 260, 512)
DS = NARROW + WIDE
NS = (24, 23)                                # 16-byte rows (the vector forms) / not (guarded loads, fp32 MFMA when narrow)
ROWS = ((1, 1), (3, 7), (1, 37))             # B, L: 1, 21 and 37 rows
EPS = 1e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a ROCm device"
    return torch.device("cuda:0")


def _want_form(N, D, x_bs, x_mis, w_mis):
    if D > 128:
        return embed_wide_rule(N, D, x_bs, x_mis, w_mis)
    return embed_rule(N, D, x_bs, x_mis, w_mis, **SW_E)


def _setup(ftn, dev, B, L, N, D, seed, scale=1.0):
    """A contiguous window, the weight, and the form the library reports for them (asserted against the rule)."""
    g = torch.Generator().manual_seed(seed)
    flat, off, st = _window(B, L, N, "plain", g, scale)
    w = torch.randn(D, N, generator=g) / N ** 0.5
    win = _as_window(flat, off, st, B, L, N)
    win_d, w_d = _as_window(flat.to(dev), off, st, B, L, N), w.to(dev)
    form = ftn.runtime.embed_form(win_d, w_d)
    assert form == _want_form(N, D, st[0] if B > 1 else 0, win_d.data_ptr() & 15, w_d.data_ptr() & 15)
    vec = N % 4 == 0
    if D > 128:
        assert form.startswith("k_embed_wide_bf<") and form.endswith("true>" if vec else "false>")
    elif not vec:
        assert form == f"k_embed_in<{4 if D <= 64 else 8},false>"             # guarded loads, fp32 MFMA
    else:
        assert form.startswith("k_embed_in<") if SW_E["f32"] else form.startswith("k_embed_in_bf<")
    return g, win, w, win_d, w_d, form


def _params(D, g):
    return torch.rand(D, generator=g) + 0.5, torch.randn(D, generator=g)


def _rms64(v, gamma, beta, eps=EPS):
    v = v.double()
    return (v * torch.rsqrt(v.square().mean(dim=-1, keepdim=True) + eps)) * gamma.double() + beta.double()


def _norm_d(gamma, beta, dev):
    return gamma.to(dev), beta.to(dev), EPS, "rms"


# --------------------------------------------------------------------------------------------- epilogue against fp64
@pytest.mark.parametrize("N", NS, ids=["vec", "generic"])
@pytest.mark.parametrize("D", DS)
def test_epilogue_against_fp64(D, N, ftn, dev):
    rt = ftn.runtime
    worst = 0.0
    for (B, L) in ROWS:
        for add_mode in (None, "shared", "batch"):
            g, win, w, win_d, w_d, form = _setup(ftn, dev, B, L, N, D, seed=100 * D + 10 * N + B * L)
            add = None if add_mode is None else torch.randn(B if add_mode == "batch" else 1, L, D, generator=g)
            gamma, beta = _params(D, g)
            v = win.double() @ w.double().t()
            want = _rms64(v if add is None else v + add.double(), gamma, beta)
            got = rt.embed_forward(win_d, w_d, None if add is None else add.to(dev), _norm_d(gamma, beta, dev)).cpu()
            err = float(((got.double() - want).abs() / (2e-5 + 2e-5 * want.abs())).max())
            worst = max(worst, err)
            np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=2e-5, atol=2e-5,
                                       err_msg=str((form, B, L, N, D, add_mode)))
    print(f"RMS_EPILOGUE D={D} N={N}: worst {worst:.3f} of rtol 2e-5 / atol 2e-5")


# ------------------------------------------------------------------------------------------ ring == one pass, bitwise
@pytest.mark.parametrize("N", NS, ids=["vec", "generic"])
@pytest.mark.parametrize("D", DS)
def test_ring_equals_one_pass_bit_for_bit(D, N, ftn, dev):
    """Every head slot of an L = 5 ring with B = 5, add absent, shared and per batch row: against fp64 at the epilogue
    tolerance, and ``torch.equal`` to ``embed_forward`` of the rolled window."""
    rt = ftn.runtime
    B, L = 5, 5
    g, win, w, win_d, w_d, form = _setup(ftn, dev, B, L, N, D, seed=7000 + D + N)
    gamma, beta = _params(D, g)
    norm = _norm_d(gamma, beta, dev)
    V = torch.empty(B, L, D, device=dev)
    rt.embed_rows_strided(win_d, w_d, V, 0)
    for add in (None, torch.randn(1, L, D, generator=g), torch.randn(B, L, D, generator=g)):
        add_d = None if add is None else add.to(dev)
        for head in range(L):
            got = rt.embed_ring(V, head, add_d, norm)
            v = torch.roll(V.cpu().double(), -head, dims=1)
            want = _rms64(v if add is None else v + add.double(), gamma, beta)
            np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), rtol=2e-5, atol=2e-5)
            rolled = torch.roll(win_d, -head, dims=1).contiguous()
            assert torch.equal(got, rt.embed_forward(rolled, w_d, add_d, norm)), (form, head, add is not None)


# ------------------------------------------------------------------------------------------------------ row properties
@pytest.mark.parametrize("N,D", [(24, 36), (23, 128), (24, 132), (23, 512)])
def test_row_bits_do_not_depend_on_the_batch(N, D, ftn, dev):
    rt = ftn.runtime
    g = torch.Generator().manual_seed(N + D)
    x = torch.randn(150, 1, N, generator=g).to(dev)                     # 150 rows of L = 1: more than one workgroup
    w = (torch.randn(D, N, generator=g) / N ** 0.5).to(dev)
    add = torch.randn(1, 1, D, generator=g).to(dev)
    gamma, beta = _params(D, g)
    norm = _norm_d(gamma, beta, dev)
    full = rt.embed_forward(x, w, add, norm)
    for r in (0, 17, 63, 64, 127, 128, 149):
        assert torch.equal(rt.embed_forward(x[r:r + 1], w, add, norm), full[r:r + 1]), r
    assert torch.equal(rt.embed_forward(x[140:], w, add, norm), full[140:])
    assert torch.equal(rt.embed_forward(x[3:40], w, add, norm), full[3:40])
    as_window = rt.embed_forward(x[2:150].reshape(4, 37, N), w, add.expand(1, 37, D).contiguous(), norm)
    assert torch.equal(as_window.reshape(148, 1, D), full[2:150])        # the same rows as 4 windows of 37


@pytest.mark.parametrize("N,D", [(24, 64), (23, 100), (24, 260), (23, 512)])
def test_zero_row_gives_beta(N, D, ftn, dev):
    rt = ftn.runtime
    g = torch.Generator().manual_seed(D)
    B, L = 2, 9
    x = torch.randn(B, L, N, generator=g).to(dev)
    x[1, 4] = 0.0
    w = (torch.randn(D, N, generator=g) / N ** 0.5).to(dev)
    gamma, beta = _params(D, g)
    norm = _norm_d(gamma, beta, dev)
    out = rt.embed_forward(x, w, None, norm)
    assert torch.equal(out[1, 4], beta.to(dev))
    V = torch.empty(B, L, D, device=dev)
    rt.embed_rows_strided(x, w, V, 0)
    assert torch.equal(rt.embed_ring(V, 0, None, norm), out)
    assert torch.equal(rt.embed_forward(torch.zeros_like(x), w, None, norm), beta.to(dev).expand(B, L, D))


@pytest.mark.parametrize("N,D", [(24, 64), (23, 100), (24, 260), (23, 512)])
def test_overflowing_row_gives_beta_as_the_fp32_module_does(N, D, ftn, dev):
    """A row scaled to 1e20: its squares overflow fp32, ``1 / sqrt(inf) = 0`` and the row is beta exactly - what
    the fp32 ``RMSNorm`` module (the reference's formula, torch ops) returns on the device for the same values.  The
    other rows keep their bits."""
    rt = ftn.runtime
    g = torch.Generator().manual_seed(D + 1)
    B, L = 2, 9
    x = torch.randn(B, L, N, generator=g).to(dev)
    w = (torch.randn(D, N, generator=g) / N ** 0.5).to(dev)
    gamma, beta = _params(D, g)
    norm = _norm_d(gamma, beta, dev)
    clean = rt.embed_forward(x, w, None, norm)
    x[1, 4] *= 1e20
    v = rt.embed_forward(x, w, None, None)
    assert bool(v[1, 4].isfinite().all()) and float(v[1, 4].abs().max()) > 1e19
    out = rt.embed_forward(x, w, None, norm)
    assert torch.equal(out[1, 4], beta.to(dev))
    module = ftn.models.shell.RMSNorm(D, eps=EPS).to(dev)
    with torch.no_grad():
        module.weight.copy_(gamma)
        module.bias.copy_(beta)
        assert torch.equal(module(v)[1, 4], beta.to(dev))
    V = torch.empty(B, L, D, device=dev)
    rt.embed_rows_strided(x, w, V, 0)
    assert torch.equal(rt.embed_ring(V, 0, None, norm), out)
    out[1, 4] = clean[1, 4]
    assert torch.equal(out, clean)


@pytest.mark.parametrize("D", [64, 260])
def test_one_nan_poisons_its_own_row_only(D, ftn, dev):
    rt = ftn.runtime
    B, L, N = 3, 23, 24
    g, win, w, win_d, w_d, form = _setup(ftn, dev, B, L, N, D, seed=5000 + D)
    add = torch.randn(1, L, D, generator=g).to(dev)
    gamma, beta = _params(D, g)
    norm = _norm_d(gamma, beta, dev)
    clean = rt.embed_forward(win_d, w_d, add, norm).cpu()
    for b, l, n in [(0, 0, 0), (1, 11, N // 2), (2, L - 1, N - 1)]:
        keep = win_d[b, l, n].clone()
        win_d[b, l, n] = float("nan")
        got = rt.embed_forward(win_d, w_d, add, norm).cpu()
        win_d[b, l, n] = keep
        assert bool(got[b, l].isnan().all()), (form, b, l, n)
        got[b, l] = clean[b, l]
        assert torch.equal(got, clean), (form, b, l, n)


@pytest.mark.parametrize("N,D", [(24, 100), (23, 36), (24, 132), (23, 260)])
def test_all_four_entry_points_write_only_their_output(N, D, ftn, dev):
    """The output sits between guard words in one allocation: the guards are intact and the output is the runtime's."""
    rt, lib = ftn.runtime, ftn.lib.load()
    B, L = 1, 37
    g, win, w, win_d, w_d, form = _setup(ftn, dev, B, L, N, D, seed=9000 + D)
    add = torch.randn(1, L, D, generator=g).to(dev)
    gamma, beta = _params(D, g)
    norm = _norm_d(gamma, beta, dev)
    want = rt.embed_forward(win_d, w_d, add, norm)
    V = torch.empty(B, L, D, device=dev)
    rt.embed_rows_strided(win_d, w_d, V, 0)
    want_ring = rt.embed_ring(V, 3, add, norm)
    wide = "_wide" if D > 128 else ""
    stream = torch.cuda.current_stream(dev).cuda_stream
    n, pad = B * L * D, 256
    for which in ("forward", "ring"):
        buf = torch.full((pad + n + pad,), 1234.5, device=dev)
        out = buf[pad:pad + n]
        assert out.data_ptr() % 16 == 0
        entry = f"ftn_embed{wide}_{which}_rms"
        if which == "forward":
            rc = getattr(lib, entry)(win_d.data_ptr(), 0, B, L, N, w_d.data_ptr(), D, add.data_ptr(), 0,
                                     norm[0].data_ptr(), norm[1].data_ptr(), EPS, out.data_ptr(), stream)
        else:
            rc = getattr(lib, entry)(V.data_ptr(), B, L, D, 3, add.data_ptr(), 0, norm[0].data_ptr(),
                                     norm[1].data_ptr(), EPS, out.data_ptr(), stream)
        ftn.lib.check(rc, entry)
        torch.cuda.synchronize()
        assert bool((buf[:pad] == 1234.5).all()) and bool((buf[pad + n:] == 1234.5).all()), entry
        assert torch.equal(out.view(B, L, D), want if which == "forward" else want_ring), entry


# --------------------------------------------------------------------------------------------------------------- model
def test_reference_rms_checkpoint_runs_on_the_hip_shell(ftn, dev):
    """``dropin_rms_recursive``: state dict, inputs, rate and dispersion as the reference wrote them."""
    cfg, _ = SHELL_CASES["rms_recursive"]
    z = _fixture("rms_recursive")
    x, kw = torch.from_numpy(z["x"]), _part(z, "kw:")
    with torch.no_grad():
        torch.manual_seed(1)
        net = ftn.models.TimesNet(**cfg).eval()
        net(x, **kw)
        net.load_state_dict(_part(z, "sd:"), strict=True)
    net = net.to(dev)
    with torch.inference_mode():
        rate, disp = net(x.to(dev), **{k: v.to(dev) for k, v in kw.items()})
    assert net.embedding.embed_norm_mode == "rms"
    assert (net._last_embed_backend, net._last_context_backend, net._last_timeproj_backend,
            net._last_head_backend) == ("hip", "hip", "hip", "hip")
    assert net.period_selector.last_selected_periods.tolist() == z["periods"].tolist()
    want_r, want_d = torch.from_numpy(z["rate"]), torch.from_numpy(z["disp"])
    err = lambda a, b: float(((a.cpu() - b).abs() / (ATOL + RTOL * b.abs())).max())
    print(f"RMS_MODEL_ERR rate {err(rate, want_r):.3f} disp {err(disp, want_d):.3f} of rtol 1e-4 / atol 2e-5")
    np.testing.assert_allclose(rate.cpu().numpy(), want_r.numpy(), rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(disp.cpu().numpy(), want_d.numpy(), rtol=RTOL, atol=ATOL)


def test_graphed_forward_of_a_direct_rms_model_equals_eager(ftn, dev):
    N, L = 32, 16
    model = _model(ftn, dev, 64, N, L, 0, "rms", mode="direct")
    x, kw = _inputs(dev, 3, L, N, 4, 0, seed=5)
    x2 = x.flip(0) * 1.25
    with torch.inference_mode():
        want = [t.clone() for t in model(x, **kw)]
        want2 = [t.clone() for t in model(x2, **kw)]
    assert model._last_embed_backend == "hip"
    model._last_embed_backend = "unset"
    gf = ftn.graph.GraphedForward(model, x, **kw)
    got = [t.clone() for t in gf(x, **kw)]
    got2 = [t.clone() for t in gf(x2, **kw)]
    torch.cuda.synchronize()
    assert model._last_embed_backend == "hip"
    assert all(torch.equal(a, b) for a, b in zip(got, want)) and all(torch.equal(a, b) for a, b in zip(got2, want2))
    assert not torch.equal(want[0], want2[0])


# ---------------------------------------------------------------------------------------------------- device forecasts
def _no_loop(*a, **k):
    raise AssertionError("the host loop ran: the device path did not take this forecast")


@pytest.mark.parametrize("marks", [0, 2], ids=["plain", "marks"])
@pytest.mark.parametrize("N", [32, 37])
@pytest.mark.parametrize("d_model", [36, 64, 128, 192])
def test_device_forecasts_equal_the_loop(d_model, N, marks, ftn, dev, monkeypatch):
    F = ftn.forecast
    L, T, B, H, P = 16, 20, 3, 20, 3
    model = _model(ftn, dev, d_model, N, L, marks, "rms")
    assert model.embedding.embed_norm_mode == "rms"
    x, kw = _inputs(dev, B, T, N, H, marks, seed=5)
    marks_kw = {k: kw[k] for k in ("x_mark", "y_mark") if k in kw}
    with torch.inference_mode():
        want_r, want_d = _loop(model, x, H, **kw)
        want_p = model.period_selector.last_selected_periods.tolist()
        want_s = F.forecast_sample_paths_loop(model, x, H, P, seed=7, **kw)
        with monkeypatch.context() as mp:
            mp.setattr(F, "forecast_recursive_batch_loop", _no_loop)
            mp.setattr(F, "forecast_sample_paths_loop", _no_loop)
            got_r, got_d = F.forecast_recursive_batch(model, x, H, **kw)
            got_p = model.period_selector.last_selected_periods.tolist()
            assert (model._last_embed_backend, model._last_head_backend) == ("hip", "hip")
            fc = F.RecursiveForecaster(model, x, H, **kw)
            rep_r, rep_d = (t.clone() for t in fc(x, **marks_kw))
            got_s = F.forecast_sample_paths(model, x, H, P, seed=7, **kw)
    torch.cuda.synchronize()
    assert got_r.shape == (B, H, N)
    assert torch.equal(got_r, want_r) and torch.equal(got_d, want_d) and got_p == want_p
    assert torch.equal(rep_r, got_r) and torch.equal(rep_d, got_d)
    assert all(a.shape == (P, B, H, N) and torch.equal(a, b) for a, b in zip(got_s, want_s))


# ---------------------------------------------------------------------------------------------------- the switch forms
@pytest.mark.parametrize("switch", ["FTN_EMBED_F32=1", "FTN_EMBED_RT=1", "FTN_EMBED_RT=2"])
def test_epilogue_and_ring_under_switch(switch):
    """The embedding's other forms (the library reads the switches once: a fresh child process).  Ring == one pass must
    hold on them too - that is why ``forecast._prepare`` needs no form list for "rms"."""
    name, value = switch.split("=")
    env = dict(os.environ, **{name: value})
    r = subprocess.run([sys.executable, "-m", "pytest", str(Path(__file__).resolve()), "-m", "gpu", "-x", "-q",
                        "-k", "test_epilogue_against_fp64 or test_ring_equals_one_pass_bit_for_bit"],
                       env=env, capture_output=True, text=True, timeout=600, cwd=str(ROOT))
    tail = (r.stdout + r.stderr)[-1500:]
    assert r.returncode == 0, tail
    assert " passed" in r.stdout and "failed" not in r.stdout, tail
