"""The TimesBlock kernels on a workspace whose old content is unknown (``include/flowtimes.h`` at
``ftn_timesblock_workspace_bytes``, DESIGN section 1 "Workspaces"): the result of a block call does not depend on the
bytes the workspace held before it, for any bit pattern, and the call writes nothing outside the workspace.

Nothing clears a workspace and ``runtime._workspace`` hands it out as ``torch.empty``, so every region must be written
before it is read and every reader must mask the rest: tail pixels, padded channels, the pad row, the pixels of a
launch bound beyond the descriptor's.  The other block tests call one block on one shape several times, so the caching
allocator hands a later call the values an identical earlier call left behind, and a forgotten write stays hidden.
Here every call gets a workspace filled with one of ``ws_poison.PATTERNS`` between two guards (``tests/ws_poison.py``).

Shapes, parameters, stubs, fp64 references and tolerances are those of ``test_gpu_forms.py`` and
``test_gpu_forms_small.py``, by import: the smallest shapes at which each form exists.  ``HYGIENE_SMALL`` /
``HYGIENE_WIDE`` / ``HYGIENE_HALF`` are the case tables; ``test_ws_poison_host.py`` checks on the CPU that they name
every form of ``SMALL_FORMS`` and ``TABLE_FORMS``."""
import ctypes

import numpy as np
import pytest
import torch

import test_gpu_forms as wide
import test_gpu_forms_small as small
from test_gpu_forms import ATOL, LN_ATOL, LN_RTOL, RTOL, _Stub, _check, expected_forms
from test_gpu_forms_small import (SMALL_BASE, SMALL_HALF, STUB_TILED, TILED_ROWS, WIDE, _block, _stub, _stub_amps,
                                  expected_forms_small)
from ws_poison import PATTERNS, check_guards, pattern_tensor, poisoned_workspace

pytestmark = pytest.mark.gpu

SELECTORS = ("native", "stub")
# (C, d_ff, ratio, kernel set, engine, selector): every fp32 row of SMALL_FORMS under both selectors, then TILED_ROWS
HYGIENE_SMALL = [b + (s,) for b in SMALL_BASE for s in SELECTORS] + [r + ("tiled",) for r in TILED_ROWS]
# (C, engine, selector): the d_model 64 / 128 rows of test_gpu_forms, native selector at L = 336 and the 7-group stub
HYGIENE_WIDE = [(C, e, s) for C in wide.WIDTHS for e in wide.ENGINES for s in SELECTORS]
HYGIENE_HALF = [b + (dt,) for b in SMALL_HALF for dt in ("bfloat16", "float16")]
SENTINEL = -12345.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a ROCm device"
    return torch.device("cuda:0")


def _layernorm(C, dev):
    ln = torch.nn.LayerNorm(C).to(dev)
    with torch.no_grad():
        ln.weight.copy_(torch.linspace(0.5, 1.5, C))
        ln.bias.copy_(torch.linspace(-0.2, 0.2, C))
    return ln


def _strip(forms):
    return {k: v for k, v in forms.items() if k != "spectrum"}


def _call(blk, xd, ln, engine):
    """``y``, ``y_ln`` and the forms of both calls; for f16x2 the pending range words are resolved first (a repair
    would rewrite ``y``) and must show no trip."""
    with torch.inference_mode():
        y = blk(xd)
        forms = blk._last_forms
        y_ln = blk(xd, post_norm=ln)
        forms_ln = blk._last_forms
        used = blk.check_range()
    torch.cuda.synchronize()
    assert blk._last_backend == "hip"
    if engine == "f16x2":
        assert blk._range_fallbacks == 0 and used == "f16x2" and blk._last_engine_used == "f16x2" and not blk._range_pending
    return y, y_ln, forms, forms_ln


def _four_runs(ftn, monkeypatch, blk, xd, ln, engine, want):
    """The block under each pattern and once on an untouched ``_workspace``: returns the zero-pattern ``(y, y_ln)``
    after asserting bit equality across the four runs, the forms of every call, the guards, and that x and the packed
    weights are as they were."""
    wblob = blk._packed(xd.device)[0]
    x0, w0 = xd.clone(), wblob.clone()
    runs = {}
    for p in PATTERNS:
        log = []
        with monkeypatch.context() as m:
            m.setattr(ftn.runtime, "_workspace", poisoned_workspace(p, log))
            runs[p] = _call(blk, xd, ln, engine)
        assert len(log) >= 2, "the block did not allocate through runtime._workspace"
        check_guards(log)
        assert _strip(runs[p][2]) == want and _strip(runs[p][3]) == want
    plain = _call(blk, xd, ln, engine)
    assert _strip(plain[2]) == want and _strip(plain[3]) == want
    assert blk._packed(xd.device)[0] is wblob
    assert torch.equal(xd, x0) and torch.equal(wblob, w0)
    diffs = []
    for p in PATTERNS:
        for i, what in ((0, "y"), (1, "y_ln")):
            a, b = runs[p][i], plain[i]
            if not torch.equal(a, b):
                bad = a != b                                     # (NaN != anything: a NaN on either side counts)
                idx = bad.nonzero()
                diffs.append(f"{what} under workspace pattern {p:#04x} differs from the unpatched run at "
                             f"{int(bad.sum())} of {a.numel()} elements ({int(a.isnan().sum())} NaN), first [b, t, c] = "
                             f"{idx[0].tolist()}, last {idx[-1].tolist()}: {float(a[tuple(idx[0])])} vs "
                             f"{float(b[tuple(idx[0])])}")
    assert not diffs, "\n".join(diffs)
    return runs[0x00][0], runs[0x00][1]


def _fp64_criterion(y, y_ln, y_ref, ln, engine):
    C = y_ref.shape[-1]
    err = _check(y, y_ref, engine, RTOL, ATOL)
    ln_ref = torch.nn.functional.layer_norm(y_ref, (C,), ln.weight.detach().double().cpu(),
                                            ln.bias.detach().double().cpu(), ln.eps)
    return err, _check(y_ln, ln_ref, engine, LN_RTOL, LN_ATOL)


# ---- a. every form under every pattern
@pytest.mark.parametrize("C,d_ff,ratio,ks,engine,selector", HYGIENE_SMALL)
def test_small_forms_ignore_old_workspace_content(C, d_ff, ratio, ks, engine, selector, ftn, dev, monkeypatch):
    P, x, y_ref, periods = small._reference(C, d_ff, ratio, ks, "gelu", selector)
    blk = _block(ftn, C, d_ff, ratio, ks, engine, "gelu", dev)
    B, L, _ = x.shape
    if selector == "native":
        blk.period_selector = ftn.models.timesnet.FFTPeriodSelector(small.NATIVE[C >= WIDE]["K"], L)
    else:
        object.__setattr__(blk, "period_selector", _Stub(periods, _stub_amps(_stub(C, selector))))
    if selector == "tiled":
        assert (B, L) == (STUB_TILED["B"], STUB_TILED["L"])
    xd = x.to(dev)
    assert xd.data_ptr() % 16 == 0
    ln = _layernorm(C, dev)
    fused = selector == "native" and ftn.runtime.fuse_stage_a(blk._packed(dev)[1])
    want = expected_forms_small(C, d_ff, ratio, ks, engine, "gelu", 0, True, fused)
    y, y_ln = _four_runs(ftn, monkeypatch, blk, xd, ln, engine, want)
    if selector == "native":
        assert blk.period_selector.last_selected_periods.tolist() == periods
    err, err_ln = _fp64_criterion(y, y_ln, y_ref, ln, engine)
    print(f"ws_hygiene B={B} L={L} C={C} d_ff={d_ff} ratio={ratio} {ks} {engine} {selector}: {want['A']} {want['conv']} "
          f"{want['C']} {want['E']} max|y-y64|={err:.3e} ln {err_ln:.3e} patterns equal")


@pytest.mark.parametrize("C,engine,selector", HYGIENE_WIDE)
def test_d64_d128_forms_ignore_old_workspace_content(C, engine, selector, ftn, dev, monkeypatch):
    P, x, y_ref, periods = wide._reference(C, "gelu", selector)
    T = ftn.models.timesnet
    blk = T.TimesBlock(C, wide.KS, 0.0, "gelu", d_ff=4 * C, bottleneck_ratio=4.0)
    blk.engine = engine
    blk.inception.load_state_dict(P, strict=True)
    blk = blk.eval().to(dev)
    B, L, _ = x.shape
    if selector == "native":
        assert L == wide.NATIVE["L"] == 336
        blk.period_selector = T.FFTPeriodSelector(wide.NATIVE["K"], L)
    else:
        assert len(periods) == 7
        object.__setattr__(blk, "period_selector", _Stub(periods, wide._stub_amps()))
    xd = x.to(dev)
    assert xd.data_ptr() % 16 == 0
    ln = _layernorm(C, dev)
    fused = selector == "native" and ftn.runtime.fuse_stage_a(blk._packed(dev)[1])
    want = expected_forms(C, engine, "gelu", 0, True, fused)
    y, y_ln = _four_runs(ftn, monkeypatch, blk, xd, ln, engine, want)
    if selector == "native":
        assert blk.period_selector.last_selected_periods.tolist() == periods
    err, err_ln = _fp64_criterion(y, y_ln, y_ref, ln, engine)
    print(f"ws_hygiene B={B} L={L} C={C} d_ff={4 * C} ratio=4.0 k357 {engine} {selector}: {want['A']} {want['conv']} "
          f"{want['C']} {want['E']} max|y-y64|={err:.3e} ln {err_ln:.3e} patterns equal")


# ---- b. the forms only a half input reaches
@pytest.mark.parametrize("C,d_ff,ratio,ks,engine,dtype", HYGIENE_HALF)
def test_half_input_forms_ignore_old_workspace_content(C, d_ff, ratio, ks, engine, dtype, ftn, dev, monkeypatch):
    dtype = getattr(torch, dtype)
    n = small.NATIVE[C >= WIDE]
    blk = _block(ftn, C, d_ff, ratio, ks, engine, "gelu", dev)
    blk.period_selector = ftn.models.timesnet.FFTPeriodSelector(n["K"], n["L"])
    x = torch.from_numpy(ftn.synth.make_input(n["B"], n["L"], C, seed=n["seed"], planted=n["planted"])).to(dev)
    x16 = x.to(dtype)
    adt = ftn.runtime.ACT_DTYPE[dtype]
    want = expected_forms_small(C, d_ff, ratio, ks, engine, "gelu", adt, True, ftn.runtime.fuse_stage_a(blk._packed(dev)[1]))

    def call():
        with torch.inference_mode():
            y = blk(x16)
            forms = blk._last_forms
            used = blk.check_range()
        torch.cuda.synchronize()
        assert blk._last_backend == "hip" and y.dtype == dtype and _strip(forms) == want
        if engine == "f16x2":
            assert blk._range_fallbacks == 0 and used == "f16x2"
        return y

    runs = {}
    for p in PATTERNS:
        log = []
        with monkeypatch.context() as m:
            m.setattr(ftn.runtime, "_workspace", poisoned_workspace(p, log))
            runs[p] = call()
        assert log
        check_guards(log)
    y16 = call()
    for p in PATTERNS:
        assert torch.equal(runs[p], y16), f"y under workspace pattern {p:#04x} differs from the unpatched run"
    with torch.inference_mode():
        y32 = blk(x)
    np.testing.assert_allclose(y16.float().cpu().numpy(), y32.cpu().numpy(), rtol=0.05, atol=0.1)
    print(f"ws_hygiene B={n['B']} L={n['L']} C={C} d_ff={d_ff} ratio={ratio} {ks} {engine} {dtype} native: {want['A']} "
          f"{want['conv']} {want['C']} {want['E']} max|y16-y32|={float((y16.float() - y32).abs().max()):.3e} "
          f"patterns equal")


# ---- c. the C entry points with loose and exact bounds
@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("C,d_ff,ratio,ks,engine,stage_e", [
    (64, 256, 4.0, "k357", "f16x2", "k_out_h<2>"), (24, 96, 4.0, "k357", "f32", "k_out_fast"),
    (16, 16, 1.0, "k3", "f32", "k_out_merged"), (128, 512, 4.0, "k357", "f32", "k_out"),
])
def test_entry_points_do_not_depend_on_the_launch_bounds(C, d_ff, ratio, ks, engine, stage_e, norm, ftn, dev):
    """A pixel's arithmetic does not depend on ``max_groups`` / ``px_bound``; the regions a loose bound adds to the
    workspace are touched by no kernel, or masked by every reader."""
    lib, rt = ftn.lib.load(), ftn.runtime
    B, L, periods = 3, 50, [49, 7, 16]
    blk = _block(ftn, C, d_ff, ratio, ks, engine, "gelu", dev)
    wblob, plan = blk._packed(dev)
    forms = rt.timesblock_forms(plan, B, L, 0, 0)
    assert forms["E"] == stage_e
    x = torch.from_numpy(ftn.synth.make_input(B, L, C, seed=55, planted=())).to(dev)
    dh = ftn.lib.desc_from_periods(periods, L, 1, L)
    G, px = int(dh.n_groups), int(dh.total_px)
    assert G == 3
    w = torch.softmax(torch.from_numpy(np.random.RandomState(55).standard_normal(size=(B, 3)).astype(np.float32)), 1)
    sel = rt.selection_from_host(dh, w, dev)
    assert (sel.max_groups, sel.px_bound) == (G, px)
    gamma, beta = torch.linspace(0.5, 1.5, C, device=dev), torch.linspace(-0.2, 0.2, C, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    # exact; between the two (odd, no multiple of a 16-pixel unit); the worst case, nearly 2 L max_groups pixels a row
    bounds = [(G, px), (7, 2 * px + 1), (ftn.lib.FTN_KMAX, 0)]
    needs, ys, log = [], [], []
    for mg, pxb in bounds:
        need = lib.ftn_timesblock_workspace_bytes(ctypes.byref(plan), B, L, mg, pxb)
        assert need > 0
        ws = poisoned_workspace(0xFF, log)(dev, need)
        y = torch.full_like(x, SENTINEL)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        if norm:
            rc = lib.ftn_timesblock_forward_norm(x.data_ptr(), y.data_ptr(), B, L, ctypes.byref(plan), wblob.data_ptr(),
                                                 sel.desc.data_ptr(), sel.weights.data_ptr(), mg, pxb, 0, gamma.data_ptr(),
                                                 beta.data_ptr(), 1e-5, ws.data_ptr(), ws.numel(), st, flag.data_ptr())
        else:
            rc = lib.ftn_timesblock_forward(x.data_ptr(), y.data_ptr(), B, L, ctypes.byref(plan), wblob.data_ptr(),
                                            sel.desc.data_ptr(), sel.weights.data_ptr(), mg, pxb, 0, 0, ws.data_ptr(),
                                            ws.numel(), st, flag.data_ptr())
        ftn.lib.check(rc, "ftn_timesblock_forward")
        torch.cuda.synchronize()
        assert int(flag.item()) == 0, f"range word set under bounds {(mg, pxb)}"
        assert not bool((y == SENTINEL).any()), f"y not fully written under bounds {(mg, pxb)}"
        assert bool(torch.isfinite(y).all()), f"y not finite under bounds {(mg, pxb)}"
        needs.append(need)
        ys.append(y)
    check_guards(log)
    assert needs[0] < needs[1] < needs[2]
    assert torch.equal(ys[1], ys[0]) and torch.equal(ys[2], ys[0])
    print(f"ws_hygiene bounds B={B} L={L} C={C} {engine} norm={norm}: {forms['A']} {forms['conv']} {forms['C']} "
          f"{forms['E']} workspace bytes {needs} bounds equal")


# ---- d. the selection buffers runtime.finalize leaves as torch.empty
DESC_SCALARS = ("n_sel", "n_groups", "total_px", "tiles_per_row")
DESC_PER_SEL = ("sel_freq", "sel_period", "sel_group")
DESC_PER_GROUP = ("g_period", "g_pad", "g_cycles", "g_px_off", "g_tw", "g_th", "g_ntx", "g_nty", "g_tile_off")


def _desc_fields(ftn, desc):
    d = ftn.lib.FtnDesc.from_buffer_copy(desc.cpu().numpy().tobytes())
    out = {f: int(getattr(d, f)) for f in DESC_SCALARS}
    n, G = out["n_sel"], out["n_groups"]
    assert 0 <= n <= ftn.lib.FTN_KMAX and 0 <= G <= ftn.lib.FTN_KMAX
    out.update({f: list(getattr(d, f))[:n] for f in DESC_PER_SEL})
    out.update({f: list(getattr(d, f))[:G] for f in DESC_PER_GROUP})
    return out


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("B,L,C,K,d_ff,engine", [(5, 97, 24, 3, 96, "f32"), (3, 96, 64, 5, 256, "f16x2")])
def test_selection_buffers_ignore_their_old_content(B, L, C, K, d_ff, engine, fused, ftn, dev, monkeypatch):
    """``ftn_period_finalize`` / ``ftn_period_finalize_stage_a`` into ``desc``, ``amps``, ``wts`` that hold each
    pattern, then the block on that selection: what the kernels read of the three buffers, and y, do not depend on it.
    Nothing is asserted about the entries beyond ``n_sel`` / ``n_groups``."""
    lib, rt = ftn.lib.load(), ftn.runtime
    KMAX = ftn.lib.FTN_KMAX
    blk = _block(ftn, C, d_ff, 4.0, "k357", engine, "gelu", dev)
    wblob, plan = blk._packed(dev)
    assert rt.fuse_stage_a(plan)
    selector = ftn.models.timesnet.FFTPeriodSelector(K, L)
    k, pmax, thr = int(selector.k), int(selector.pmax), int(selector.min_period_threshold)
    x = torch.from_numpy(ftn.synth.make_input(B, L, C, seed=57)).to(dev)
    med, psum = rt.spectrum(x)
    mg, pxb = rt._selector_bounds(lib, L, k, pmax, thr)
    need = rt._workspace_bytes(lib, plan, B, L, mg, pxb)
    st = torch.cuda.current_stream().cuda_stream
    got = {}
    for p in PATTERNS:
        log = []
        desc = pattern_tensor(p, (ftn.lib.DESC_INTS,), torch.int32, dev)
        amps = pattern_tensor(p, (B, KMAX), torch.float32, dev)
        wts = pattern_tensor(p, (B, KMAX), torch.float32, dev)
        sel = rt.Selection(desc, amps, wts, mg, pxb)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        if fused:
            ws = poisoned_workspace(p, log)(dev, need)
            rc = lib.ftn_period_finalize_stage_a(psum.data_ptr(), 1, B, med.data_ptr(), B, L, k, pmax, thr, 0, 0, 0.0,
                                                 desc.data_ptr(), amps.data_ptr(), wts.data_ptr(), x.data_ptr(),
                                                 ctypes.byref(plan), wblob.data_ptr(), mg, pxb, ws.data_ptr(), ws.numel(),
                                                 st, flag.data_ptr(), None)
            ftn.lib.check(rc, "ftn_period_finalize_stage_a")
            sel.stage_a = rt.StageA(x, plan, wblob, flag, ws)
        else:
            rc = lib.ftn_period_finalize(psum.data_ptr(), 1, B, med.data_ptr(), B, L, k, pmax, thr, 0, 0, 0.0,
                                         desc.data_ptr(), amps.data_ptr(), wts.data_ptr(), st, None)
            ftn.lib.check(rc, "ftn_period_finalize")
        with monkeypatch.context() as m, torch.inference_mode():
            m.setattr(rt, "_workspace", poisoned_workspace(p, log))   # (the block's own, where stage A was not fused)
            y = rt.timesblock_forward(x, plan, wblob, sel, range_flag=flag)
        torch.cuda.synchronize()
        assert len(log) == 1
        check_guards(log)
        assert int(flag.item()) == 0 and bool(torch.isfinite(y).all())
        got[p] = (_desc_fields(ftn, desc), amps.cpu(), wts.cpu(), y)
    f0, a0, w0, y0 = got[PATTERNS[0]]
    n, G = f0["n_sel"], f0["n_groups"]
    assert 1 <= G <= n == K < KMAX
    for p in PATTERNS[1:]:
        f, a, w, y = got[p]
        assert f == f0, (hex(p), f, f0)
        assert torch.equal(a[:, :n], a0[:, :n]) and torch.equal(w[:, :G], w0[:, :G]), hex(p)
        assert torch.equal(y, y0), f"y on selection buffers pre-filled with {p:#04x} differs from the zero-filled run"
    print(f"ws_hygiene selection B={B} L={L} C={C} K={K} {engine} fused={fused}: n_sel={n} n_groups={G} "
          f"periods={f0['g_period']} patterns equal")


# ---- e. whole model and one recursive forecast
@pytest.mark.parametrize("name", ["m_pipeline", "m_context"])
def test_full_model_ignores_old_workspace_content(name, manifest, golden, ftn, dev, monkeypatch):
    import test_gpu_parity as parity

    case, g = manifest[name], golden(name)
    model, kw = parity._model_from_fixture(ftn, case, g, dev)
    x = torch.from_numpy(g["x"]).to(dev)
    with torch.inference_mode():
        rate, disp = model(x, **kw)
    torch.cuda.synchronize()
    log = []
    with monkeypatch.context() as m:
        m.setattr(ftn.runtime, "_workspace", poisoned_workspace(0xFF, log))
        with torch.inference_mode():
            rate_p, disp_p = model(x, **kw)
        torch.cuda.synchronize()
    assert all(b._last_backend == "hip" for b in model.blocks)
    assert len(log) >= len(model.blocks)                          # one per block (its own, or its fused stage A's)
    check_guards(log)
    assert torch.equal(rate_p, rate) and torch.equal(disp_p, disp)
    np.testing.assert_allclose(rate_p.cpu().numpy(), g["rate"], rtol=parity.RTOL, atol=parity.ATOL)
    np.testing.assert_allclose(disp_p.cpu().numpy(), g["dispersion"], rtol=parity.RTOL, atol=parity.ATOL)
    print(f"ws_hygiene model {name}: {len(log)} workspaces over {len(model.blocks)} blocks, patterns equal")


def test_recursive_forecast_ignores_old_workspace_content(ftn, dev, monkeypatch):
    import test_gpu_recursive as rec

    d_model, N, L, T, B, _, marks, norm = rec.FORECASTS["d64_plain_b1"]
    H = 6
    model = rec._model(ftn, dev, d_model, N, L, marks, norm)
    x, kw = rec._inputs(dev, B, T, N, H, marks, seed=5)
    with torch.inference_mode():
        rate, disp = ftn.forecast.forecast_recursive_batch(model, x, H, **kw)
    torch.cuda.synchronize()
    log = []
    with monkeypatch.context() as m:
        m.setattr(ftn.runtime, "_workspace", poisoned_workspace(0xFF, log))
        with torch.inference_mode():
            rate_p, disp_p = ftn.forecast.forecast_recursive_batch(model, x, H, **kw)
        torch.cuda.synchronize()
    assert model._last_embed_backend == "hip" and all(b._last_backend == "hip" for b in model.blocks)
    assert len(log) >= H * len(model.blocks)
    check_guards(log)
    assert rate_p.shape == (B, H, N)
    assert torch.equal(rate_p, rate) and torch.equal(disp_p, disp)
    print(f"ws_hygiene forecast d64_plain_b1 H={H}: {len(log)} workspaces, patterns equal")
