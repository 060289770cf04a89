"""The time projection on the MI355X (``ftn_timeproj_forward``: ``k_timeproj_bf`` for S > 1, ``k_timeproj_row`` for
S == 1): accuracy against fp64 under the a-priori bound of the shell GEMMs, bit-identity of a row across batch sizes,
writes confined to the output, the model forward (direct and recursive) against its CPU mirror, graph replay,
recursive forecasting against the host loop, and the series-sharded hidden rows.

Measured (MI355X, the whole case table below; e in units of u = 2^-24 as defined in ``_err_u``, bound L + 8):
    k_timeproj_bf   max e = 6.09 u at L = 1 (bound 9 u)   (fp32 torch.matmul on the CPU, its cases: 5.48 u)
    k_timeproj_row  max e = 3.52 u at L = 31 (bound 39 u)  (fp32 torch.matmul on the CPU, its cases: 4.01 u)
"""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-4, 2e-5          # the model-level tolerance of tests/test_gpu_parity.py
U = 2.0 ** -24

DS = (4, 12, 36, 64, 68, 128)
LS = (1, 5, 31, 32, 33, 96, 336, 720)
SS = (1, 2, 15, 16, 17, 96)
BS = (1, 3, 64)
SCALES = (1e-6, 1.0, 1e6)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a ROCm device"
    return torch.device("cuda:0")


def _operands(B, L, S, D, sliced, scale, seed):
    """seq, W_t, b_t on the CPU.  ``sliced``: W_t / b_t are ``weight[-S:]`` / ``bias[-S:]`` of a matrix one row
    taller, so the device copy of W_t starts 4 L bytes into an allocation: off a 16-byte boundary when L % 4 != 0."""
    g = torch.Generator().manual_seed(seed)
    seq = torch.randn(B, L, D, generator=g) * scale
    rows = S + 1 if sliced else S
    weight = torch.randn(rows, L, generator=g) / L ** 0.5
    bias = torch.randn(rows, generator=g) * scale
    return seq, weight, bias


def _err_u(got, seq, wt, bt):
    """DESIGN section 4's metric for the shell GEMMs: |got - ref64| / (sum_l |W_t[s,l]| |seq[b,l,d]| + |b_t[s]|), in
    units of u = 2^-24, maximised over the outputs; the reference and the denominator in fp64 on the CPU."""
    w64, s64, b64 = wt.double(), seq.double(), bt.double()
    ref = torch.matmul(w64, s64) + b64.view(1, -1, 1)
    den = torch.matmul(w64.abs(), s64.abs()) + b64.abs().view(1, -1, 1)
    den = torch.where(den > 0, den, torch.ones_like(den))
    return float(((got.double() - ref).abs() / den).max()) / U


@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("D", DS)
def test_accuracy_against_fp64(D, L, ftn, dev):
    """Every (S, B) at this (D, L); the slice / scale pair rotates so that each of the six appears with every D, L, S
    and B somewhere in the table.  Asserted: e <= L + 8 (the (K + 8) u rule of the embedding and heads with K = L; a
    lost piece product would show as ~256 u).  Printed beside it: the same e of fp32 torch.matmul on the CPU."""
    rt = ftn.runtime
    worst = {}
    for (si, S), (bi, B) in itertools.product(enumerate(SS), enumerate(BS)):
        combo = (3 * si + bi + DS.index(D) + 5 * LS.index(L)) % 6
        sliced, scale = bool(combo & 1), SCALES[combo >> 1]
        seq, weight, bias = _operands(B, L, S, D, sliced, scale, seed=1000 * D + 10 * L + S + B)
        wt, bt = weight[-S:], bias[-S:]
        dw, db = weight.to(dev)[-S:], bias.to(dev)[-S:]
        dseq = seq.to(dev)
        form = rt.timeproj_form(dseq, dw)
        assert form.startswith("k_timeproj_row" if S == 1 else "k_timeproj_bf"), form
        if sliced and L % 4:
            assert dw.data_ptr() % 16 != 0 and (S == 1 or form.endswith("false>"))
        got = rt.timeproj_forward(dseq, dw, db)
        assert got.shape == (B, S, D) and got.is_contiguous()
        e = _err_u(got.cpu(), seq, wt, bt)
        e_cpu = _err_u(torch.matmul(wt, seq) + bt.view(1, -1, 1), seq, wt, bt)
        key = form.split("<")[0]
        worst[key] = max(worst.get(key, (0.0, 0.0)), (e, e_cpu))
        assert e <= L + 8, (form, B, L, S, D, sliced, scale, e)
    for key, (e, e_cpu) in sorted(worst.items()):
        print(f"TIMEPROJ_ERR D={D} L={L} {key} e={e:.3f}u cpu_fp32_matmul={e_cpu:.3f}u bound={L + 8}u")


@pytest.mark.parametrize("S", [1, 2, 17, 96, 100])
@pytest.mark.parametrize("D,L", [(64, 336), (128, 720), (36, 33), (12, 5), (68, 96)])
def test_row_is_bit_identical_in_any_batch(D, L, S, ftn, dev):
    """Row b of a B-row call = the 1-row call on seq[b:b+1] = its row in the call on seq[b0:b1], bit for bit."""
    rt = ftn.runtime
    B = 7
    seq, weight, bias = _operands(B, L, S, D, True, 1.0, seed=D + L + S)
    dseq, dw, db = seq.to(dev), weight.to(dev)[-S:], bias.to(dev)[-S:]
    full = rt.timeproj_forward(dseq, dw, db)
    for b in range(B):
        assert torch.equal(rt.timeproj_forward(dseq[b:b + 1], dw, db), full[b:b + 1]), b
    assert torch.equal(rt.timeproj_forward(dseq[2:5], dw, db), full[2:5])
    assert torch.equal(rt.timeproj_forward(dseq[3:], dw, db), full[3:])
    big = torch.cat([dseq, dseq.flip(0)] * 20)                 # 280 rows: more workgroups than a first wave of them
    got = rt.timeproj_forward(big, dw, db)
    assert torch.equal(got[:B], full) and torch.equal(got[-B:], full.flip(0))
    assert torch.equal(rt.timeproj_forward(dseq, dw, db), full)   # and the same bits on a second run


@pytest.mark.parametrize("B,L,S,D", [(3, 33, 17, 12), (2, 5, 15, 68), (5, 31, 1, 36), (1, 96, 1, 4), (2, 40, 100, 100),
                                     (3, 720, 2, 128)])
def test_writes_only_its_output(B, L, S, D, ftn, dev):
    """hidden sits between guard words in one allocation: they are untouched, and the interior is what the wrapper
    returns for the same operands."""
    rt = ftn.runtime
    seq, weight, bias = _operands(B, L, S, D, True, 1.0, seed=B + L + S + D)
    dseq, dw, db = seq.to(dev), weight.to(dev)[-S:], bias.to(dev)[-S:]
    n, pad = B * S * D, 256
    buf = torch.full((pad + n + pad,), 1234.5, device=dev)
    hid = buf[pad:pad + n]
    assert hid.data_ptr() % 16 == 0
    rc = rt._lib.load().ftn_timeproj_forward(dseq.data_ptr(), B, L, D, dw.data_ptr(), db.data_ptr(), S, hid.data_ptr(),
                                             torch.cuda.current_stream(dev).cuda_stream)
    rt.check(rc, "ftn_timeproj_forward")
    torch.cuda.synchronize()
    assert bool((buf[:pad] == 1234.5).all()) and bool((buf[pad + n:] == 1234.5).all())
    assert torch.equal(hid.view(B, S, D), rt.timeproj_forward(dseq, dw, db))
    assert e_ok(hid.view(B, S, D).cpu(), seq, weight[-S:], bias[-S:], L)


def e_ok(got, seq, wt, bt, L):
    return _err_u(got, seq, wt, bt) <= L + 8


# ------------------------------------------------------------------------------------------------------- model level
def _mirrors(ftn, dev, mode, d_model, ctx, N=24, L=24, H=6, seed=0):
    """The same TimesNet on the CPU (torch path) and on the device, lazily built parts woken up."""
    cfg = dict(input_len=L, pred_len=H, d_model=d_model, d_ff=2 * d_model, n_layers=2, k_periods=3,
               kernel_set=[(3, 3), (5, 5)], dropout=0.0, activation="gelu", mode=mode, use_checkpoint=False)
    if ctx:
        cfg.update(id_embed_dim=4, use_zero_mean_context=True, context_rank=4)
    g = torch.Generator().manual_seed(seed + 1)
    kw = {"series_ids": torch.arange(N), "series_static": torch.randn(N, 3, generator=g)} if ctx else {}
    torch.manual_seed(seed)
    cpu = ftn.models.TimesNet(**cfg).eval()
    with torch.no_grad():
        cpu(torch.rand(2, L, N, generator=g) + 1.0, **kw)
        for p in cpu.parameters():                              # wake the zero-initialised heads / context maps
            if float(p.abs().sum()) == 0.0:
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
    gpu = ftn.models.TimesNet(**cfg).eval()
    dkw = {k: v.to(dev) for k, v in kw.items()}
    with torch.no_grad():
        gpu(torch.ones(2, L, N, device=dev), **dkw)
    gpu.load_state_dict(cpu.state_dict(), strict=True)
    t = torch.arange(L, dtype=torch.float32).view(1, L, 1)
    x = torch.rand(5, L, N, generator=g) + 1.5 + torch.sin(2 * torch.pi * t / 6.0)
    return cpu, gpu, x, kw, dkw


@pytest.mark.parametrize("ctx", [False, True], ids=["plain", "static_ids"])
@pytest.mark.parametrize("d_model", [64, 128])
@pytest.mark.parametrize("mode", ["direct", "recursive"])
def test_model_forward_matches_its_cpu_mirror(mode, d_model, ctx, ftn, dev):
    cpu, gpu, x, kw, dkw = _mirrors(ftn, dev, mode, d_model, ctx)
    assert cpu._last_timeproj_backend == "torch"
    with torch.no_grad():
        want_r, want_d = cpu(x, **kw)
    assert cpu._last_timeproj_backend == "torch"
    with torch.inference_mode():
        rate, disp = gpu(x.to(dev), **dkw)
    assert gpu._last_timeproj_backend == "hip" and gpu._last_head_backend == "hip"
    assert gpu.period_selector.last_selected_periods.tolist() == cpu.period_selector.last_selected_periods.tolist()
    assert rate.shape == (5, 6 if mode == "direct" else 1, 24)
    np.testing.assert_allclose(rate.cpu().numpy(), want_r.numpy(), rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(disp.cpu().numpy(), want_d.numpy(), rtol=RTOL, atol=ATOL)


def test_autograd_path_stays_on_torch(ftn, dev):
    _, gpu, x, _, _ = _mirrors(ftn, dev, "direct", 64, False)
    with torch.inference_mode():
        gpu(x.to(dev))
    assert gpu._last_timeproj_backend == "hip"
    gpu(x.to(dev))                                              # grad enabled, parameters require grad
    assert gpu._last_timeproj_backend == "torch"


@pytest.mark.parametrize("mode,d_model", [("direct", 64), ("direct", 128), ("recursive", 64)])
def test_graph_replay_is_bit_equal_to_eager(mode, d_model, ftn, dev):
    _, gpu, x, _, dkw = _mirrors(ftn, dev, mode, d_model, True)
    x = x.to(dev)
    x2 = x.flip(0) * 1.25
    with torch.inference_mode():
        want = [t.clone() for t in gpu(x, **dkw)]
        want2 = [t.clone() for t in gpu(x2, **dkw)]
    gf = ftn.graph.GraphedForward(gpu, x, **dkw)
    got = [t.clone() for t in gf(x, **dkw)]
    got2 = [t.clone() for t in gf(x2, **dkw)]
    torch.cuda.synchronize()
    assert gpu._last_timeproj_backend == "hip"
    assert all(torch.equal(a, b) for a, b in zip(got, want)) and all(torch.equal(a, b) for a, b in zip(got2, want2))
    assert not torch.equal(want[0], want2[0])


@pytest.mark.parametrize("d_model,ctx", [(64, True), (128, False)])
def test_recursive_forecasts_stay_bit_equal_to_the_loop(d_model, ctx, ftn, dev):
    """The row form is on both sides: the device path, the captured forecaster and the host loop agree bit for bit."""
    F = ftn.forecast
    _, gpu, x, _, dkw = _mirrors(ftn, dev, "recursive", d_model, ctx)
    x, H = x.to(dev), 20
    with torch.inference_mode():
        want_r, want_d = F.forecast_recursive_batch_loop(gpu, x, H, **dkw)
        assert gpu._last_timeproj_backend == "hip" and gpu._last_head_backend == "hip"
        got_r, got_d = F.forecast_recursive_batch(gpu, x, H, **dkw)
        assert gpu._last_timeproj_backend == "hip"
        rep_r, rep_d = F.RecursiveForecaster(gpu, x, H, **dkw)(x)
    torch.cuda.synchronize()
    assert got_r.shape == (5, H, 24)
    assert torch.equal(got_r, want_r) and torch.equal(got_d, want_d)
    assert torch.equal(rep_r, want_r) and torch.equal(rep_d, want_d)


@pytest.mark.parametrize("mode,d_model", [("direct", 64), ("direct", 128), ("recursive", 128)])
def test_series_hidden_of_half_the_batch_equals_rows_of_the_full_call(mode, d_model, ftn, dev):
    """What a rank of the series-sharded forward computes for its B/2 rows is the full-batch call's rows."""
    _, gpu, _, _, _ = _mirrors(ftn, dev, mode, d_model, False)
    steps = 6 if mode == "direct" else 1
    g = torch.Generator().manual_seed(3)
    seq = torch.randn(8, 24, d_model, generator=g).to(dev)
    with torch.inference_mode():
        full = gpu.series_hidden(seq, steps)
        assert gpu._last_timeproj_backend == "hip" and full.shape == (8, steps, d_model)
        lo, hi = gpu.series_hidden(seq[:4], steps), gpu.series_hidden(seq[4:], steps)
    assert torch.equal(lo, full[:4]) and torch.equal(hi, full[4:])
    wt, bt = gpu.forecast_time_proj.weight.detach()[-steps:], gpu.forecast_time_proj.bias.detach()[-steps:]
    assert e_ok(full.cpu(), seq.cpu(), wt.cpu(), bt.cpu(), 24)
