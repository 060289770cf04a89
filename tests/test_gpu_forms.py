"""The d_model 64 / 128 kernel forms outside the parity suite's slice (GELU, fp32 inputs, 16-byte-aligned x): ReLU,
every engine, contiguous but misaligned x, native selector and a multi-group stub - each case against the fp64 oracle,
and each case asserting which forms ran (``TimesBlock._last_forms``), so a dispatch change cannot quietly leave a form
untested.  ``FORMS_MATRIX`` / ``expected_forms`` are also what the CPU test ``test_forms_table.py`` pins the dispatch
query to.  Half-precision inputs at these widths are pinned by the reference's own fixtures (``half_wide`` in
``tests/golden/manifest_env.json``, ``test_env_flags.py``).

Tolerances: rtol 1e-4 / atol 5e-6 against the fp64 oracle (the fp32 oracle itself is ~5-8e-7 from it at these
shapes; the split engines agree with f32 within 5e-6, ``test_engines_agree_and_plain_bf16_is_close``); the plain
bf16 engine keeps its reduced-precision criterion, max error below 5 % of max |y|."""
import functools
import itertools

import numpy as np
import pytest
import torch

from oracle import timesblock_oracle as orc

KS = [(3, 3), (5, 5), (7, 7)]
NS = {"f32": 0, "bf16x3": 3, "f16x2": 2, "bf16": 1}
ENGINES = tuple(NS)
WIDTHS = (64, 128)
ACTS = ("gelu", "relu")
ALIGNS = ("aligned", "misaligned")
# native selector: planted periods, L = 336, K = 5.  Stub: 7 groups (both position-major forms need several passes),
# pads 60 (four tail units), 4, 4, 6, 3, 2, 11; L % 16 != 0; odd B
NATIVE = dict(B=3, L=336, K=5, seed=41)
STUB = dict(B=3, L=150, periods=[70, 7, 11, 13, 17, 19, 23], seed=42)
SELECTORS = ("native", "stub")
RTOL, ATOL = 1e-4, 5e-6
LN_RTOL, LN_ATOL = 1e-4, 1e-5


def expected_forms(C, engine, act, act_dtype=0, aligned=True, fused_a=False):
    """The dispatch table of ``forward_t`` at the pipeline kernel set (3x3, 5x5, 7x7), ratio 4, d_ff 4 C."""
    ns = NS[engine]
    rk = rs = False
    if ns == 0:
        conv, stage_c, stage_e = "k_conv", "k_mlp", "k_out_fast" if C == 64 else "k_out"
    elif C == 64:
        conv = f"k_conv_bf_fast<{ns},1>"
        if act_dtype == 0:
            stage_c, rk, rs = f"k_mlp_pos64<{ns}>", True, True
            stage_e = f"k_out_h<{ns}>" if ns >= 2 else "k_out_fast"
        else:
            stage_c, stage_e = f"k_mlp_bf_u1<{ns}>", "k_out_fast"
    else:
        conv = "k_conv_bf_fast<2,2>" if ns == 2 else f"k_conv_bf<2,{ns}>"
        if act_dtype == 0 and ns == 2:
            stage_c, rk, rs, stage_e = "k_mlp_pos128<2>", True, True, "k_out_h<2>"
        else:
            stage_c = f"k_mlp_bf_c128<{ns}>"
            stage_e = f"k_out_h<{ns}>" if act_dtype == 0 and ns == 3 else "k_out"
    epi = 0 if ns == 0 else (3 if ns == 2 else 2)
    return {"act": act, "xvec": bool(aligned), "yvec": True, "A": f"k_finalize_pw<{epi}>" if fused_a else f"k_pw<1,{epi}>",
            "conv": conv, "C": stage_c, "r_keeps_x": rk, "r_summed": rs, "E": stage_e, "half_round": act_dtype != 0}


# (C, engine, act, act_dtype, aligned): fp32 inputs in both alignments here; half inputs (always handed to the
# kernels as a fresh aligned fp32 copy) through the half_wide fixtures
FORMS_MATRIX = ([(C, e, a, 0, al == "aligned") for C, e, a, al in itertools.product(WIDTHS, ENGINES, ACTS, ALIGNS)] +
                [(C, e, a, adt, True) for C, e, a, adt in itertools.product(WIDTHS, ("f16x2", "f32"), ACTS, (1, 2))])
# the rows of the table: (C, engine, input) -> (conv, stage C, stage E)
TABLE_FORMS = {
    (64, "f16x2", "fp32"): ("k_conv_bf_fast<2,1>", "k_mlp_pos64<2>", "k_out_h<2>"),
    (64, "bf16x3", "fp32"): ("k_conv_bf_fast<3,1>", "k_mlp_pos64<3>", "k_out_h<3>"),
    (64, "bf16", "fp32"): ("k_conv_bf_fast<1,1>", "k_mlp_pos64<1>", "k_out_fast"),
    (64, "f16x2", "half"): ("k_conv_bf_fast<2,1>", "k_mlp_bf_u1<2>", "k_out_fast"),
    (64, "f32", "any"): ("k_conv", "k_mlp", "k_out_fast"),
    (128, "f16x2", "fp32"): ("k_conv_bf_fast<2,2>", "k_mlp_pos128<2>", "k_out_h<2>"),
    (128, "bf16x3", "fp32"): ("k_conv_bf<2,3>", "k_mlp_bf_c128<3>", "k_out_h<3>"),
    (128, "f16x2", "half"): ("k_conv_bf_fast<2,2>", "k_mlp_bf_c128<2>", "k_out"),
}


def _params(C, act):
    import __graft_entry__ as ge
    ftn = ge.load_package()
    return {k: torch.from_numpy(v) for k, v in ftn.synth.make_inception_params(C, 4 * C, KS, 4.0, seed=C + (act == "relu")).items()}


def _input(C, selector):
    import __graft_entry__ as ge
    ftn = ge.load_package()
    if selector == "native":
        return torch.from_numpy(ftn.synth.make_input(NATIVE["B"], NATIVE["L"], C, seed=NATIVE["seed"]))
    return torch.from_numpy(ftn.synth.make_input(STUB["B"], STUB["L"], C, seed=STUB["seed"], planted=()))


def _stub_amps():
    return np.random.RandomState(STUB["seed"]).standard_normal(size=(STUB["B"], len(STUB["periods"]))).astype(np.float32)


def oracle_fp64(x, P, act, k, L, periods=None, amps=None, ks=KS):
    """The block in fp64: periods chosen by the fp32 oracle selector on fp32 x (as the seeded parity tests do), then
    ``orc.timesblock_forward`` on double x / parameters / amplitudes with those periods (kernel set ``ks``)."""
    if periods is None:
        sel = orc.period_select(x, k, L, 1)
        periods, amps = sel.periods, sel.amps
    y, _ = orc.timesblock_forward(x.double(), {n: v.double() for n, v in P.items()}, ks, act, 0, L, 1,
                                  periods=list(periods), amps=torch.as_tensor(amps).double())
    return y, list(periods)


@functools.lru_cache(maxsize=None)
def _reference(C, act, selector):
    P, x = _params(C, act), _input(C, selector)
    if selector == "native":
        y, periods = oracle_fp64(x, P, act, NATIVE["K"], NATIVE["L"])
    else:
        y, periods = oracle_fp64(x, P, act, 0, STUB["L"], STUB["periods"], _stub_amps())
    return P, x, y, periods


class _Stub(torch.nn.Module):
    def __init__(self, periods, amps):
        super().__init__()
        self.periods = torch.as_tensor(periods, dtype=torch.long)
        self.amps = torch.as_tensor(amps, dtype=torch.float32)

    def forward(self, x):
        return self.periods.to(x.device), self.amps.to(device=x.device, dtype=x.dtype)


def _misaligned_copy(x):
    buf = torch.empty(x.numel() + 1, dtype=x.dtype, device=x.device)
    xm = buf[1:].view(x.shape)
    xm.copy_(x)
    assert xm.is_contiguous() and xm.data_ptr() % 16 != 0
    return xm


def _check(y, y_ref, engine, rtol, atol):
    y, y_ref = y.double().cpu(), y_ref.double()
    err = (y - y_ref).abs()
    if engine == "bf16":                                         # plain bf16 products: BASELINE configs[2]
        assert float(err.max()) < 0.05 * float(y_ref.abs().max())
    else:
        np.testing.assert_allclose(y.numpy(), y_ref.numpy(), rtol=rtol, atol=atol)
    return float(err.max())


@pytest.mark.gpu
@pytest.mark.parametrize("selector", SELECTORS)
@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("C", WIDTHS)
def test_forms_match_fp64_oracle(C, act, engine, align, selector, ftn):
    dev = torch.device("cuda:0")
    P, x, y_ref, periods = _reference(C, act, selector)
    T = ftn.models.timesnet
    blk = T.TimesBlock(C, KS, 0.0, act, d_ff=4 * C, bottleneck_ratio=4.0)
    blk.engine = engine
    blk.inception.load_state_dict(P, strict=True)
    blk = blk.eval().to(dev)
    B, L, _ = x.shape
    if selector == "native":
        blk.period_selector = T.FFTPeriodSelector(NATIVE["K"], L)
    else:
        object.__setattr__(blk, "period_selector", _Stub(periods, _stub_amps()))
    xd = x.to(dev)
    if align == "misaligned":
        xd = _misaligned_copy(xd)
    else:
        assert xd.data_ptr() % 16 == 0
    ln = torch.nn.LayerNorm(C).to(dev)
    with torch.no_grad():
        ln.weight.copy_(torch.linspace(0.5, 1.5, C))
        ln.bias.copy_(torch.linspace(-0.2, 0.2, C))
    with torch.inference_mode():
        y = blk(xd)
        forms = blk._last_forms
        y_ln = blk(xd, post_norm=ln)
        forms_ln = blk._last_forms
    assert blk._last_backend == "hip"
    fused = selector == "native" and ftn.runtime.fuse_stage_a(blk._pack[1])
    want = expected_forms(C, engine, act, 0, align == "aligned", fused)
    assert {k: v for k, v in forms.items() if k != "spectrum"} == want
    assert {k: v for k, v in forms_ln.items() if k != "spectrum"} == want
    if selector == "native":
        assert blk.period_selector.last_selected_periods.tolist() == periods
        assert forms["spectrum"] == ftn.runtime.spectrum_form(B, L, C, xd.data_ptr() % 16)
    assert blk._last_group_count == len(orc.period_group(periods, L, 1, L).periods)
    err = _check(y, y_ref, engine, RTOL, ATOL)
    ln_ref = torch.nn.functional.layer_norm(y_ref, (C,), ln.weight.detach().double().cpu(), ln.bias.detach().double().cpu(),
                                            ln.eps)
    err_ln = _check(y_ln, ln_ref, engine, LN_RTOL, LN_ATOL)
    print(f"forms C={C} {act} {engine} {align} {selector}: {want['conv']} {want['C']} {want['E']} "
          f"max|y-y64|={err:.3e} ln {err_ln:.3e}")


# ---- the selector's spectrum on misaligned x: the scalar branches of the row-resident forms against the float4 ones
@pytest.mark.gpu
@pytest.mark.parametrize("B,L,C,form", [(64, 336, 64, "k_spectrum_rowq"), (64, 250, 64, "k_spectrum_row"),
                                        (3, 336, 128, "k_spectrum_rowq_tiled"), (64, 720, 128, "k_spectrum_rowq_tiled")])
def test_spectrum_misaligned_matches_aligned(B, L, C, form, ftn):
    dev = torch.device("cuda:0")
    x = torch.from_numpy(ftn.synth.make_input(B, L, C, seed=43)).to(dev)
    xm = _misaligned_copy(x)
    assert ftn.runtime.spectrum_form(B, L, C, 0) == (form, True)
    assert ftn.runtime.spectrum_form(B, L, C, xm.data_ptr() % 16) == (form, False)
    med_a, psum_a = ftn.runtime.spectrum(x)
    med_m, psum_m = ftn.runtime.spectrum(xm)
    np.testing.assert_allclose(med_m.cpu().numpy(), med_a.cpu().numpy(), rtol=1e-5, atol=0)
    np.testing.assert_allclose(psum_m.cpu().numpy(), psum_a.cpu().numpy(), rtol=1e-5, atol=0)
    T = ftn.models.timesnet
    sel = T.FFTPeriodSelector(5, L)
    with torch.inference_mode():
        pa = sel(x)[0].tolist()
        pm = sel(xm)[0].tolist()
    assert pa == pm == orc.period_select(x.cpu(), 5, L, 1).periods
