"""Row passes on the MI355X (DESIGN §4 "Row passes"): a TimesBlock call of any batch size runs stages A-F over its one
selection in passes of rows through a workspace of one pass, and the bits are those of a single pass.

  1  B = 65 540 (beyond the one-shot row limit) against the oracle and the full-batch selector
  2  B = 7 in passes of 1 .. 8 rows against the one-shot call, bit for bit, per stage-C family, engine and input dtype
  3  the f16x2 range guard with the offending row in a middle pass
  4  a captured two-layer TimesNet under FTN_ROWS_PER_PASS
  5  sample paths with P * B > 65 535
  6  the channel-tiled selector form beyond 65 535 rows
  7  k_row_weights (FTN_FIN_ROWS forced, child processes) against the finalize workgroup's own row loop

Shapes come from the tables of ``test_gpu_forms.py`` / ``test_gpu_forms_small.py`` and ``_last_forms`` is asserted as
those tests assert it, so a pass runs the forms the table names."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import timesblock_oracle as orc
from test_gpu_forms import KS, expected_forms
from test_gpu_forms_small import KSETS, SMALL_FORMS

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
RTOL, ATOL = 1e-4, 2e-5                    # the suite's bound against the fp32 oracle (test_gpu_parity.py)
BIG_B = 65540
ROWS = (1, 2, 3, 6, 7, 8)                  # passes of B = 7: ragged last passes (2, 3, 6), one row, exactly B, more than B


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a ROCm device"
    return torch.device("cuda:0")


def _block(ftn, dev, C, d_ff, ratio, ks, act, engine, K, L, seed):
    T = ftn.models.timesnet
    blk = T.TimesBlock(C, ks, 0.0, act, d_ff=d_ff, bottleneck_ratio=ratio)
    blk.engine = engine
    P = {k: torch.from_numpy(v) for k, v in ftn.synth.make_inception_params(C, d_ff, ks, ratio, seed).items()}
    blk.inception.load_state_dict(P, strict=True)
    blk.period_selector = T.FFTPeriodSelector(K, L)
    return blk.eval().to(dev), P


def _strip(forms):
    return {k: v for k, v in forms.items() if k != "spectrum"}


# ------------------------------------------------------------------------------------------------ 1: beyond 65 535 rows
def test_block_beyond_the_row_limit(ftn, dev):
    """d_model 16, d_ff 64, kernels 3/5/7 (a row of the small forms table), L = 12, k = 2, B = 65 540: two passes by
    default.  Fails without row passes: the library rejects the shape."""
    C, d_ff, ratio, L, K = 16, 64, 4.0, 12, 2
    assert (C, d_ff, ratio, "k357", "f16x2", 0) in SMALL_FORMS
    blk, P = _block(ftn, dev, C, d_ff, ratio, KSETS["k357"], "gelu", None, K, L, seed=7)
    g = torch.Generator().manual_seed(11)
    t = torch.arange(L, dtype=torch.float32).view(1, L, 1)
    a = 0.5 + torch.rand(BIG_B, 1, C, generator=g)
    x = (a * torch.sin(2 * torch.pi * t / 6.0) + 0.6 * a.flip(2) * torch.cos(2 * torch.pi * t / 4.0)
         + 0.05 * torch.randn(BIG_B, L, C, generator=g)).contiguous()
    sel = orc.period_select(x, K, L)
    xd = x.to(dev)
    with torch.inference_mode():
        y = blk(xd)
        assert blk._last_backend == "hip" and blk._last_passes == (2, 65535)
        assert blk.check_range() == "f16x2"
        forms = blk._last_forms
        idx = blk.period_selector.last_frequency_indices.tolist()
        periods = blk.period_selector.last_selected_periods.tolist()
        amps = blk.period_selector(xd)[1].cpu()
        blk.rows_per_pass = 20000
        y2 = blk(xd)
        assert blk._last_passes == (4, 20000) and blk.check_range() == "f16x2"
    assert idx == sel.freq_idx and periods == sel.periods            # bit-exact against the full batch
    a_, conv, stage_c, rk, rs, stage_e = SMALL_FORMS[(C, d_ff, ratio, "k357", "f16x2", 0)]
    assert (forms["A"], forms["conv"], forms["C"], forms["E"]) == (a_, conv, stage_c, stage_e)     # no fused stage A
    assert forms["spectrum"] == ftn.runtime.spectrum_form(BIG_B, L, C, 0)
    rows = [0, 65534, 65535, 65536, 65539]
    y_ref, _ = orc.timesblock_forward(x[rows], P, KSETS["k357"], "gelu", K, L, periods=periods, amps=amps[rows])
    got = y[rows].cpu().numpy()
    print(f"row passes B={BIG_B}: max|y-ref| on rows {rows} = {np.abs(got - y_ref.numpy()).max():.3e}")
    np.testing.assert_allclose(got, y_ref.numpy(), rtol=RTOL, atol=ATOL)
    assert torch.equal(y2, y)


# ------------------------------------------------------------------------------------ 2: same bits as one pass (B = 7)
# one shape per stage-C family: the d_model-64 position-major shape at a short L, the d_model-128 shape, generic wide
# shapes (k_pw_chain: two rows of the small table, since no single one lists all three engines)
FAMILIES = [("pos64", 64, 256, 4.0, "k357", e) for e in ("f32", "bf16x3", "f16x2")] + \
           [("c128", 128, 512, 4.0, "k357", e) for e in ("f32", "bf16x3", "f16x2")] + \
           [("wide", 100, 200, 1.5, "k35", "f32"), ("wide", 72, 144, 1.5, "k3579", "bf16x3"),
            ("wide", 72, 144, 1.5, "k3579", "f16x2")]
DTYPES = {0: torch.float32, 1: torch.bfloat16, 2: torch.float16}


def _want(family, C, d_ff, ratio, ks, engine, adt, fused_a):
    if family != "wide":
        return expected_forms(C, engine, "gelu", adt, True, fused_a)
    a, conv, stage_c, rk, rs, stage_e = SMALL_FORMS[(C, d_ff, ratio, ks, engine, 0)]      # half inputs: the same forms
    assert stage_c == "k_pw_chain"
    if fused_a:
        a = a.replace("k_pw<1,", "k_finalize_pw<")
    return {"act": "gelu", "xvec": True, "yvec": True, "A": a, "conv": conv, "C": stage_c, "r_keeps_x": rk,
            "r_summed": rs, "E": stage_e, "half_round": adt != 0}


@pytest.mark.parametrize("family,C,d_ff,ratio,ks,engine", FAMILIES)
def test_passes_give_the_bits_of_one_pass(family, C, d_ff, ratio, ks, engine, ftn, dev):
    B, L, K = 7, 48, 3
    kset = KS if ks == "k357" else KSETS[ks]
    assert kset == KSETS[ks]
    blk, _ = _block(ftn, dev, C, d_ff, ratio, kset, "gelu", engine, K, L, seed=C)
    x = torch.from_numpy(ftn.synth.make_input(B, L, C, seed=21, planted=(12, 8, 6))).to(dev)
    ln = torch.nn.LayerNorm(C).to(dev)
    with torch.no_grad():
        ln.weight.copy_(torch.linspace(0.5, 1.5, C))
        ln.bias.copy_(torch.linspace(-0.2, 0.2, C))
    fuse = ftn.runtime.fuse_stage_a(blk._packed(dev)[1])
    with torch.inference_mode():
        for adt, dtype in DTYPES.items():
            xin = x.to(dtype)
            for norm in ((None, ln) if adt == 0 else (None,)):
                blk.rows_per_pass = None
                want = blk(xin, post_norm=norm)
                assert blk._last_backend == "hip" and blk._last_passes == (1, B)
                assert _strip(blk._last_forms) == _want(family, C, d_ff, ratio, ks, engine, adt, fuse)
                for rows in ROWS:
                    blk.rows_per_pass = rows
                    got = blk(xin, post_norm=norm)
                    n = min(rows, B)
                    assert blk._last_passes == ((1, B) if rows >= B else (-(-B // n), n))
                    assert _strip(blk._last_forms) == _want(family, C, d_ff, ratio, ks, engine, adt, fuse and rows >= B)
                    assert got.dtype == want.dtype and torch.equal(got, want), (adt, norm is not None, rows)
        blk.check_range()
    assert blk._range_fallbacks == 0


def test_workspace_cap_bounds_the_pass(ftn, dev):
    """``workspace_cap_bytes``: the pass is the largest whose workspace fits, the bits are unchanged, and a cap below
    one row is a ValueError that names the bytes."""
    B, L, K, C = 7, 48, 3, 64
    blk, _ = _block(ftn, dev, C, 256, 4.0, KS, "gelu", None, K, L, seed=C)
    x = torch.from_numpy(ftn.synth.make_input(B, L, C, seed=21, planted=(12, 8, 6))).to(dev)
    rt = ftn.runtime
    _, plan = blk._packed(dev)
    mg, pxb = rt.selector_bounds(L, K, L, 1)
    ws = lambda n: int(ftn.lib.load().ftn_timesblock_workspace_bytes(plan, n, L, mg, pxb))
    with torch.inference_mode():
        want = blk(x)
        blk.workspace_cap_bytes = ws(3) + 100
        got = blk(x)
        assert blk._last_passes == (3, 3) and torch.equal(got, want)
        blk.workspace_cap_bytes = ws(1) - 1
        with pytest.raises(ValueError, match=f"{ws(1) - 1} bytes.*{ws(1)} bytes"):
            blk(x)
        blk.workspace_cap_bytes = None
        assert torch.equal(blk(x), want) and blk._last_passes == (1, B)
        blk.check_range()


# --------------------------------------------------------------------------------------------------- 3: the range guard
def test_range_guard_in_a_middle_pass(ftn, dev):
    """Passes of 3 rows of B = 7; row 4 (middle pass) at scale 1e5: the shared flag is the OR over the passes, the call
    is repeated on bf16x3 in the same passes and ends up as the all-bf16x3 chunked result, bit for bit."""
    B, L, K, C = 7, 96, 3, 64
    blk, _ = _block(ftn, dev, C, 256, 4.0, KS, "gelu", None, K, L, seed=3)
    safe, _ = _block(ftn, dev, C, 256, 4.0, KS, "gelu", "bf16x3", K, L, seed=3)
    base = ftn.synth.make_input(B, L, C, seed=6, planted=(24, 12, 8))
    base = (base / np.abs(base).max()).astype(np.float32)
    base[4] *= np.float32(1e5)
    x = torch.from_numpy(base).to(dev)
    blk.rows_per_pass = safe.rows_per_pass = 3
    with torch.inference_mode():
        want = safe(x)
        assert safe.check_range() == "bf16x3" and safe._range_fallbacks == 0 and safe._last_passes == (3, 3)
        safe.rows_per_pass = None
        assert torch.equal(safe(x), want)
        with pytest.warns(RuntimeWarning, match="fp16 range"):
            y = blk(x)
            assert blk._last_passes == (3, 3)
            assert blk._last_engine == "bf16x3"
        assert blk._range_fallbacks == 1
        assert torch.isfinite(y).all() and torch.equal(y, want)


# ------------------------------------------------------------------------------------------------- child-process helper
def _child(code, tmp_path, **env):
    script = tmp_path / "child.py"
    script.write_text(f"import sys\nsys.path.insert(0, {str(ROOT)!r})\nsys.path.insert(0, {str(ROOT / 'tests')!r})\n"
                      "import __graft_entry__ as ge\nftn = ge.load_package()\nimport torch\n" + code)
    r = subprocess.run([sys.executable, str(script)], env=dict(os.environ, **env), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


# -------------------------------------------------------------------------------------------------- 4: a captured model
_GRAPH_CHILD = """
import numpy as np
dev = torch.device("cuda:0")
KS = [(3, 3), (5, 5), (7, 7)]
cfg = dict(input_len=48, pred_len=8, d_model=64, d_ff=256, n_layers=2, k_periods=3, kernel_set=KS, dropout=0.0,
           activation="gelu", mode="direct", bottleneck_ratio=4.0)
torch.manual_seed(0)
model = ftn.models.TimesNet(**cfg).eval().to(dev)
x = (torch.from_numpy(ftn.synth.make_input(7, 48, 16, seed=3)).abs() + 0.5).to(dev)
x2 = (torch.from_numpy(ftn.synth.make_input(7, 48, 16, seed=4)).abs() + 0.5).to(dev)
g = torch.Generator().manual_seed(1)
with torch.no_grad():
    model(x[:2])
    for p in model.parameters():
        if float(p.abs().sum()) == 0.0:
            p.copy_(0.05 * torch.randn(p.shape, generator=g).to(p.device))
with torch.inference_mode():
    eager = [t.clone() for t in model(x)]
    eager2 = [t.clone() for t in model(x2)]
    passes = [b._last_passes for b in model.blocks]
    assert all(b._last_backend == "hip" for b in model.blocks), [b._last_backend for b in model.blocks]
    assert passes == [(3, 3), (3, 3)], passes
    gf = ftn.graph.GraphedForward(model, x)
    out = [t.clone() for t in gf(x)]
    out2 = [t.clone() for t in gf(x2)]
    assert [b._last_passes for b in model.blocks] == [(3, 3), (3, 3)]
for a, b in zip(eager + eager2, out + out2):
    assert torch.equal(a, b)
assert not torch.equal(eager[0], eager2[0])
print("GRAPH_OK", passes)
"""


def test_captured_model_replays_its_passes(tmp_path):
    out = _child(_GRAPH_CHILD, tmp_path, FTN_ROWS_PER_PASS="3")
    assert "GRAPH_OK [(3, 3), (3, 3)]" in out, out


# -------------------------------------------------------------------------------------------------- 5: sample paths
def test_sample_paths_beyond_the_row_limit(ftn, dev):
    """x[257, 8, 1], 256 paths: one batch of 65 792 rows per step.  Both forecasts raise without row passes."""
    from test_gpu_recursive import _inputs, _model

    fc = ftn.forecast
    B, L, N, H, P = 257, 8, 1, 2, 256
    model = _model(ftn, dev, 16, N, L, 0, "decoupled", n_layers=1)
    x, kw = _inputs(dev, B, L, N, H, 0, seed=3)
    with torch.inference_mode():
        want = fc.forecast_sample_paths_loop(model, x, H, P, seed=17, **kw)
        assert all(b._last_backend == "hip" and b._last_passes == (2, 65535) for b in model.blocks)
        model._last_embed_backend = None
        got = fc.forecast_sample_paths(model, x, H, P, seed=17, **kw)
        big = x.repeat(P, 1, 1)
        rate, disp = fc.forecast_recursive_batch(model, big, H, **kw)
        rate, disp = rate.clone(), disp.clone()
        rf = fc.RecursiveForecaster(model, big, H, **kw)             # the H steps, passes unrolled, as one graph
        r2, d2 = rf(big)
        assert torch.equal(r2, rate) and torch.equal(d2, disp)
    assert model._last_embed_backend == "hip" and all(b._last_passes == (2, 65535) for b in model.blocks)
    for g_, w_ in zip(got, want):
        assert tuple(g_.shape) == (P, B, H, N) and torch.equal(g_, w_)
    assert bool(torch.isfinite(got[0]).all())
    assert torch.equal(rate[:, 0], got[1].reshape(P * B, H, N)[:, 0])          # step 0 does not depend on the draws


# -------------------------------------------------------------------------------------------------- 6: the selector
def test_tiled_spectrum_beyond_the_row_limit(ftn, dev):
    B, L, C = BIG_B, 8, 128
    rt = ftn.runtime
    assert rt.spectrum_form(B, L, C, 0) == ("k_spectrum_rowq_tiled", True)
    g = torch.Generator(device=dev).manual_seed(5)
    x = torch.rand(B, L, C, device=dev, generator=g) - 0.5
    med, psum = rt.spectrum(x)
    rows = [0, 1, 4097, 65534, 65535, 65536, 65537, 65539]
    ref = torch.fft.rfft(x[rows].double().cpu(), dim=1).abs().median(dim=2).values
    err = float((med[rows].double().cpu() - ref).abs().max())
    print(f"tiled spectrum B={B}: max|med - fp64| on rows {rows} = {err:.3e}")
    assert err <= 2e-6
    head, _ = rt.spectrum(x[:65535].contiguous())
    assert rt.spectrum_form(65535, L, C, 0) == ("k_spectrum_rowq_tiled", True)
    assert torch.equal(med[:65535], head)
    tail, _ = rt.spectrum(x[65535:].contiguous())
    assert torch.equal(med[65535:], tail)
    assert torch.allclose(psum, med.double().sum(0), rtol=1e-12, atol=0)         # (fixed-order fp64 sums of all B rows)


# ------------------------------------------------------------------------------------------------- 7: k_row_weights
_FIN_CHILD = """
import itertools
dev = torch.device("cuda:0")
rt = ftn.runtime
L, K = 48, 5
F = L // 2 + 1
out = {}
variants = {"plain": (0, 0.0), "max_uniq": (2, 0.0), "binning": (0, 2.0)}
for B, adt, (vname, (mu, lb)) in itertools.product((1, 255, 256, 257, 1000), (0, 1, 2), variants.items()):
    g = torch.Generator().manual_seed(1000 * B + adt)
    med = (torch.rand(B, F, generator=g) * 3.0 + torch.linspace(0.0, 2.0, F).flip(0)).to(dev)
    psum = med.double().sum(0)
    sel = rt.finalize(psum, B, med, L, K, L, 1, adt, mu, lb)
    out[f"{B}/{adt}/{vname}"] = (sel.desc.cpu(), sel.amps.cpu(), sel.weights.cpu())
# degenerate selections: k = 0, every score NaN, nothing valid under the clamps (pmax below the threshold is clamped:
# one period of 1), and L = 2
for name, (B, Ld, k, pmax, thr, fill) in {"k0": (300, 48, 0, 48, 1, None), "nan": (300, 48, 5, 48, 1, float("nan")),
                                            "clamp": (300, 48, 5, 1, 7, None), "L2": (257, 2, 3, 2, 1, None)}.items():
    Fd = Ld // 2 + 1
    g = torch.Generator().manual_seed(77)
    med = torch.rand(B, Fd, generator=g).to(dev)
    if fill is not None:
        med.fill_(fill)
    sel = rt.finalize(med.double().sum(0), B, med, Ld, k, pmax, thr, 0, 0, 0.0)
    out["deg/" + name] = (sel.desc.cpu(), sel.amps.cpu(), sel.weights.cpu())
torch.cuda.synchronize()
torch.save(out, sys.argv[1] if len(sys.argv) > 1 else OUT)
print("FIN_OK", len(out))
"""


def test_row_weights_kernel_equals_the_workgroup_loop(tmp_path):
    """The same finalize calls in two child processes, FTN_FIN_ROWS=1 (k_row_weights from the first row on) and
    FTN_FIN_ROWS=0 (never): descriptor, amplitudes and weights bit for bit."""
    res = {}
    for mode in ("1", "0"):
        path = tmp_path / f"fin_{mode}.pt"
        out = _child(f"OUT = {str(path)!r}\n" + _FIN_CHILD, tmp_path, FTN_FIN_ROWS=mode)
        assert "FIN_OK 49" in out, out
        res[mode] = torch.load(path)
    assert set(res["1"]) == set(res["0"]) and len(res["1"]) == 49
    live = 0
    for key, (desc, amps, wts) in res["0"].items():
        d1, a1, w1 = res["1"][key]
        assert torch.equal(d1, desc), key
        assert torch.equal(a1.view(torch.int32), amps.view(torch.int32)), key
        assert torch.equal(w1.view(torch.int32), wts.view(torch.int32)), key
        live += int(desc[1] > 0 and float(wts.abs().sum()) > 0)
    assert live >= 45                                   # the regular cases select groups and carry weights
