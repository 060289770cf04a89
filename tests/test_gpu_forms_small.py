"""Every TimesBlock kernel form outside the d_model 64 / 128 pipeline slice of ``test_gpu_forms.py``: one entry per
distinct (stage A, conv, stage C, r_keeps_x, r_summed, stage E) tuple that a sweep of the supported shapes reaches
without an ``FTN_*`` switch (DESIGN §4 "Block forms reachable without switches").  Each entry runs against the fp64
oracle with GELU and ReLU, aligned and misaligned ``x``, the native selector and a multi-group stub, and asserts which
forms ran.  ``SMALL_MATRIX`` / ``expected_forms_small`` are also what ``test_forms_table_small.py`` pins the dispatch
query to on the CPU.  Half inputs run at one entry per tuple that only a half input reaches; a ``y`` that is not
16-byte aligned (``yvec = False``) runs through the C entry points directly.

Tolerances are those of ``test_gpu_forms.py``: rtol 1e-4 / atol 5e-6 against the fp64 oracle for the fp32-equivalent
engines, 5 % of max |y| for plain bf16, ``LN_RTOL`` / ``LN_ATOL`` behind the LayerNorm epilogue."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import timesblock_oracle as orc
from test_gpu_forms import (ACTS, ALIGNS, ATOL, LN_ATOL, LN_RTOL, RTOL, SELECTORS, _Stub, _check, _misaligned_copy,
                            oracle_fp64)

KSETS = {"k3": [(3, 3)], "k35": [(3, 3), (5, 5)], "k357": [(3, 3), (5, 5), (7, 7)], "k5": [(5, 5)],
         "rect": [(3, 5), (5, 1)], "k3579": [(3, 3), (5, 5), (7, 7), (9, 9)]}
WIDE = 192                                                       # from here on the smaller geometry (fp64 oracle time)
# native selector: planted periods, K = 3.  Stub, L = 50 (L % 16 != 0), odd B: period 49 = two wide rows with pad 48,
# 1 = a 50 x 1 grid, 7 = pad 6, 16 and 25 = no pad; wide blocks: 47 = pad 46, 5 = pad 2, 16 = no pad
NATIVE = {False: dict(B=3, L=96, K=3, planted=(24, 12, 8), seed=51), True: dict(B=2, L=48, K=3, planted=(12, 8, 6), seed=52)}
STUB = {False: dict(B=3, L=50, periods=[49, 1, 7, 16, 25], seed=53), True: dict(B=2, L=48, periods=[47, 5, 16], seed=54)}
# selector "tiled": a stub whose grids are walked in several conv tiles.  L = 400: period 399 = a 2 x 399 grid in three
# column tiles, 3 = 134 x 3 in two row tiles, 16 = 25 x 16 in two row tiles of 13 units (more than one per wave).  It runs
# the forms whose multi-tile walk nothing else reaches: k_conv_bf<4,3>, k_conv_bf<1,3> with its weight groups restaged
# (at this L the 41 slabs of k3579 do not fit beside the region buffers) and k_conv
STUB_TILED = dict(B=2, L=400, periods=[399, 3, 16], seed=56)
TILED_ROWS = [(96, 192, 1.5, "k3", "bf16x3"), (8, 16, 1.5, "k3579", "bf16x3"), (100, 200, 1.5, "k35", "f32")]

# (d_model, d_ff, ratio, kernel set, engine, act_dtype) -> (A, conv, C, r_keeps_x, r_summed, E): a literal copy of what
# the sweep found, not a restatement of block_forms.  Each row's shape is the cheapest of the sweep with d_ff != d_model
# (real res1 / res2 projections in stage C) and C % 4 == 0; one row, k_conv_bf<2,2> in front of k_mlp and k_out_fast,
# exists only with d_ff == d_model = 64.  The fast-conv k_mlp rows take the pipeline hyper at C = 16 (d_ff = 4 C)
SMALL_FORMS = {
    (8, 16, 1.0, "k3", "f32", 0): ("k_embed", "k_conv", "k_mlp", False, False, "k_out_merged"),
    (8, 16, 1.5, "k3579", "bf16", 0): ("k_pw<1,2>", "k_conv_bf<1,1>", "k_mlp", False, False, "k_out"),
    (8, 16, 1.5, "k3579", "bf16x3", 0): ("k_pw<1,2>", "k_conv_bf<1,3>", "k_mlp", False, False, "k_out"),
    (8, 16, 1.5, "k3579", "f16x2", 0): ("k_pw<1,3>", "k_conv_bf<1,2>", "k_mlp", False, False, "k_out"),
    (8, 16, 1.5, "rect", "bf16", 0): ("k_pw<1,2>", "k_conv_bf<1,1>", "k_mlp", False, False, "k_out_fast"),
    (8, 16, 1.5, "rect", "bf16x3", 0): ("k_pw<1,2>", "k_conv_bf<1,3>", "k_mlp", False, False, "k_out_fast"),
    (8, 16, 1.5, "rect", "f16x2", 0): ("k_pw<1,3>", "k_conv_bf<1,2>", "k_mlp", False, False, "k_out_fast"),
    (16, 64, 4.0, "k357", "bf16", 0): ("k_pw<1,2>", "k_conv_bf_fast<1,1>", "k_mlp", False, False, "k_out_fast"),
    (16, 64, 4.0, "k357", "bf16x3", 0): ("k_pw<1,2>", "k_conv_bf_fast<3,1>", "k_mlp", False, False, "k_out_fast"),
    (16, 64, 4.0, "k357", "f16x2", 0): ("k_pw<1,3>", "k_conv_bf_fast<2,1>", "k_mlp", False, False, "k_out_fast"),
    (32, 64, 1.5, "k3", "bf16", 0): ("k_pw<1,2>", "k_conv_bf<2,1>", "k_mlp", False, False, "k_out_fast"),
    (32, 64, 1.5, "k3", "bf16x3", 0): ("k_pw<1,2>", "k_conv_bf<2,3>", "k_mlp", False, False, "k_out_fast"),
    (32, 64, 1.5, "k3", "f16x2", 0): ("k_pw<1,3>", "k_conv_bf_fast<2,2>", "k_mlp", False, False, "k_out_fast"),
    (32, 64, 1.5, "k35", "bf16", 0): ("k_pw<1,2>", "k_conv_bf<2,1>", "k_mlp", False, False, "k_out"),
    (32, 64, 1.5, "k35", "bf16x3", 0): ("k_pw<1,2>", "k_conv_bf<2,3>", "k_mlp", False, False, "k_out"),
    (32, 64, 1.5, "k35", "f16x2", 0): ("k_pw<1,3>", "k_conv_bf_fast<2,2>", "k_mlp", False, False, "k_out"),
    (32, 64, 1.5, "rect", "f16x2", 0): ("k_pw<1,3>", "k_conv_bf<2,2>", "k_mlp", False, False, "k_out"),
    (40, 80, 1.5, "k35", "bf16", 0): ("k_pw<1,2>", "k_conv_bf<2,1>", "k_mlp_bf_u1<1>", False, False, "k_out"),
    (40, 80, 1.5, "k35", "bf16x3", 0): ("k_pw<1,2>", "k_conv_bf<2,3>", "k_mlp_bf_u1<3>", False, False, "k_out_h<3>"),
    (40, 80, 1.5, "k35", "f16x2", 0): ("k_pw<1,3>", "k_conv_bf_fast<2,2>", "k_mlp_bf_u1<2>", False, False, "k_out_h<2>"),
    (40, 80, 1.5, "rect", "f16x2", 0): ("k_pw<1,3>", "k_conv_bf<2,2>", "k_mlp_bf_u1<2>", False, False, "k_out_h<2>"),
    (40, 80, 4.0, "k357", "bf16", 0): ("k_pw<1,2>", "k_conv_bf_fast<1,1>", "k_mlp_bf<1>", False, False, "k_out_fast"),
    (40, 80, 4.0, "k357", "bf16x3", 0): ("k_pw<1,2>", "k_conv_bf_fast<3,1>", "k_mlp_bf<3>", False, False, "k_out_h<3>"),
    (40, 80, 4.0, "k357", "f16x2", 0): ("k_pw<1,3>", "k_conv_bf_fast<2,1>", "k_mlp_bf<2>", False, False, "k_out_h<2>"),
    (40, 80, 4.0, "k3579", "bf16", 0): ("k_pw<1,2>", "k_conv_bf<1,1>", "k_mlp_bf_u1<1>", False, False, "k_out"),
    (40, 80, 4.0, "k3579", "bf16x3", 0): ("k_pw<1,2>", "k_conv_bf<1,3>", "k_mlp_bf_u1<3>", False, False, "k_out_h<3>"),
    (40, 80, 4.0, "k3579", "f16x2", 0): ("k_pw<1,3>", "k_conv_bf<1,2>", "k_mlp_bf_u1<2>", False, False, "k_out_h<2>"),
    (64, 64, 1.5, "k3", "f16x2", 0): ("k_pw<1,3>", "k_conv_bf<2,2>", "k_mlp", False, False, "k_out_fast"),
    (64, 128, 1.5, "k3", "bf16", 0): ("k_pw<1,2>", "k_conv_bf<2,1>", "k_mlp_pos64<1>", True, True, "k_out_fast"),
    (64, 128, 1.5, "k3", "bf16x3", 0): ("k_pw<1,2>", "k_conv_bf<2,3>", "k_mlp_pos64<3>", True, True, "k_out_h<3>"),
    (64, 128, 1.5, "k3", "f16x2", 0): ("k_pw<1,3>", "k_conv_bf<2,2>", "k_mlp_pos64<2>", True, True, "k_out_h<2>"),
    (64, 128, 2.0, "k35", "bf16", 0): ("k_pw<1,2>", "k_conv_bf<2,1>", "k_mlp_bf<1>", False, False, "k_out"),
    (64, 128, 2.0, "k35", "bf16x3", 0): ("k_pw<1,2>", "k_conv_bf<2,3>", "k_mlp_bf<3>", False, False, "k_out_h<3>"),
    (64, 128, 2.0, "k35", "f16x2", 0): ("k_pw<1,3>", "k_conv_bf_fast<2,2>", "k_mlp_bf<2>", False, False, "k_out_h<2>"),
    (64, 128, 2.0, "rect", "f16x2", 0): ("k_pw<1,3>", "k_conv_bf<2,2>", "k_mlp_bf<2>", False, False, "k_out_h<2>"),
    (64, 128, 4.0, "k3579", "bf16", 0): ("k_pw<1,2>", "k_conv_bf<1,1>", "k_mlp_bf<1>", False, False, "k_out"),
    (64, 128, 4.0, "k3579", "bf16x3", 0): ("k_pw<1,2>", "k_conv_bf<1,3>", "k_mlp_bf<3>", False, False, "k_out_h<3>"),
    (64, 128, 4.0, "k3579", "f16x2", 0): ("k_pw<1,3>", "k_conv_bf<1,2>", "k_mlp_bf<2>", False, False, "k_out_h<2>"),
    (72, 144, 1.5, "k3579", "bf16", 0): ("k_pw<1,2>", "k_conv_bf<2,1>", "k_pw_chain", False, False, "k_out"),
    (72, 144, 1.5, "k3579", "bf16x3", 0): ("k_pw<1,2>", "k_conv_bf<2,3>", "k_pw_chain", False, False, "k_out"),
    (72, 144, 1.5, "k3579", "f16x2", 0): ("k_pw<1,3>", "k_conv_bf<2,2>", "k_pw_chain", False, False, "k_out"),
    (96, 192, 1.5, "k3", "bf16", 0): ("k_pw<1,2>", "k_conv_bf<4,1>", "k_mlp", False, False, "k_out"),
    (96, 192, 1.5, "k3", "bf16x3", 0): ("k_pw<1,2>", "k_conv_bf<4,3>", "k_mlp", False, False, "k_out"),
    (96, 192, 1.5, "k3", "f16x2", 0): ("k_pw<1,3>", "k_conv_bf<4,2>", "k_mlp", False, False, "k_out"),
    (100, 200, 1.5, "k35", "bf16", 0): ("k_pw<1,2>", "k_conv_bf<4,1>", "k_pw_chain", False, False, "k_out"),
    (100, 200, 1.5, "k35", "f16x2", 0): ("k_pw<1,3>", "k_conv_bf<4,2>", "k_pw_chain", False, False, "k_out"),
    (100, 200, 1.5, "k35", "f32", 0): ("k_pw<1,0>", "k_conv", "k_pw_chain", False, False, "k_out"),
    (128, 256, 1.5, "k3", "bf16", 0): ("k_pw<1,2>", "k_conv_bf<4,1>", "k_mlp_bf_c128<1>", False, False, "k_out"),
    (128, 256, 1.5, "k3", "bf16x3", 0): ("k_pw<1,2>", "k_conv_bf<4,3>", "k_mlp_bf_c128<3>", False, False, "k_out_h<3>"),
    (128, 256, 1.5, "k3", "f16x2", 0): ("k_pw<1,3>", "k_conv_bf<4,2>", "k_mlp_pos128<2>", True, True, "k_out_h<2>"),
    (192, 384, 1.5, "k3", "bf16x3", 0): ("k_pw<1,2>", "k_conv_bf<4,3>", "k_pw_chain", False, False, "k_out"),
    # half inputs (act_dtype 1 / 2 take the same forms): the tuples no fp32 input reaches
    (40, 80, 1.5, "k35", "bf16x3", 1): ("k_pw<1,2>", "k_conv_bf<2,3>", "k_mlp_bf_u1<3>", False, False, "k_out"),
    (40, 80, 1.5, "k35", "f16x2", 1): ("k_pw<1,3>", "k_conv_bf_fast<2,2>", "k_mlp_bf_u1<2>", False, False, "k_out"),
    (40, 80, 1.5, "rect", "f16x2", 1): ("k_pw<1,3>", "k_conv_bf<2,2>", "k_mlp_bf_u1<2>", False, False, "k_out"),
    (40, 80, 4.0, "k357", "bf16x3", 1): ("k_pw<1,2>", "k_conv_bf_fast<3,1>", "k_mlp_bf<3>", False, False, "k_out_fast"),
    (40, 80, 4.0, "k357", "f16x2", 1): ("k_pw<1,3>", "k_conv_bf_fast<2,1>", "k_mlp_bf<2>", False, False, "k_out_fast"),
    (40, 80, 4.0, "k3579", "bf16x3", 1): ("k_pw<1,2>", "k_conv_bf<1,3>", "k_mlp_bf_u1<3>", False, False, "k_out"),
    (40, 80, 4.0, "k3579", "f16x2", 1): ("k_pw<1,3>", "k_conv_bf<1,2>", "k_mlp_bf_u1<2>", False, False, "k_out"),
    (64, 128, 1.5, "k3", "bf16", 1): ("k_pw<1,2>", "k_conv_bf<2,1>", "k_mlp_bf_u1<1>", False, False, "k_out_fast"),
    (64, 128, 1.5, "k3", "bf16x3", 1): ("k_pw<1,2>", "k_conv_bf<2,3>", "k_mlp_bf_u1<3>", False, False, "k_out_fast"),
    (64, 128, 1.5, "k3", "f16x2", 1): ("k_pw<1,3>", "k_conv_bf<2,2>", "k_mlp_bf_u1<2>", False, False, "k_out_fast"),
    (64, 128, 2.0, "k35", "bf16x3", 1): ("k_pw<1,2>", "k_conv_bf<2,3>", "k_mlp_bf<3>", False, False, "k_out"),
    (64, 128, 2.0, "k35", "f16x2", 1): ("k_pw<1,3>", "k_conv_bf_fast<2,2>", "k_mlp_bf<2>", False, False, "k_out"),
    (64, 128, 2.0, "rect", "f16x2", 1): ("k_pw<1,3>", "k_conv_bf<2,2>", "k_mlp_bf<2>", False, False, "k_out"),
    (64, 128, 4.0, "k357", "bf16", 1): ("k_pw<1,2>", "k_conv_bf_fast<1,1>", "k_mlp_bf_u1<1>", False, False, "k_out_fast"),
    (64, 128, 4.0, "k357", "bf16x3", 1): ("k_pw<1,2>", "k_conv_bf_fast<3,1>", "k_mlp_bf_u1<3>", False, False, "k_out_fast"),
    (64, 128, 4.0, "k3579", "bf16x3", 1): ("k_pw<1,2>", "k_conv_bf<1,3>", "k_mlp_bf<3>", False, False, "k_out"),
    (64, 128, 4.0, "k3579", "f16x2", 1): ("k_pw<1,3>", "k_conv_bf<1,2>", "k_mlp_bf<2>", False, False, "k_out"),
    (128, 256, 1.5, "k3", "bf16x3", 1): ("k_pw<1,2>", "k_conv_bf<4,3>", "k_mlp_bf_c128<3>", False, False, "k_out"),
    (128, 256, 1.5, "k3", "f16x2", 1): ("k_pw<1,3>", "k_conv_bf<4,2>", "k_mlp_bf_c128<2>", False, False, "k_out"),
    (128, 256, 4.0, "k357", "bf16x3", 1): ("k_pw<1,2>", "k_conv_bf<2,3>", "k_mlp_bf_c128<3>", False, False, "k_out"),
}

SMALL_BASE = [k[:5] for k in SMALL_FORMS if k[5] == 0]
SMALL_HALF = [k[:5] for k in SMALL_FORMS if k[5] == 1]
# (C, d_ff, ratio, kernel set, engine, act, act_dtype, aligned): fp32 inputs with both activations and both
# alignments; half inputs (handed to the kernels as a fresh aligned fp32 copy) once per dtype
SMALL_MATRIX = ([b + (act, 0, al) for b in SMALL_BASE for act in ACTS for al in (True, False)] +
                [b + ("gelu", adt, True) for b in SMALL_HALF for adt in (1, 2)])


def expected_forms_small(C, d_ff, ratio, ks, engine, act, act_dtype=0, aligned=True, fused_a=False):
    a, conv, stage_c, rk, rs, stage_e = SMALL_FORMS[(C, d_ff, ratio, ks, engine, min(act_dtype, 1))]
    if fused_a:
        a = a.replace("k_pw<1,", "k_finalize_pw<")
    return {"act": act, "xvec": bool(aligned) and C % 4 == 0, "yvec": True, "A": a, "conv": conv, "C": stage_c,
            "r_keeps_x": rk, "r_summed": rs, "E": stage_e, "half_round": act_dtype != 0}


def _ftn():
    import __graft_entry__ as ge
    return ge.load_package()


@functools.lru_cache(maxsize=None)
def _params(C, d_ff, ratio, ks, act):
    sd = _ftn().synth.make_inception_params(C, d_ff, KSETS[ks], ratio, seed=C + (act == "relu"))
    return {k: torch.from_numpy(v) for k, v in sd.items()}


def _stub(C, selector):
    return STUB_TILED if selector == "tiled" else STUB[C >= WIDE]


def _stub_amps(s):
    return np.random.RandomState(s["seed"]).standard_normal(size=(s["B"], len(s["periods"]))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _reference(C, d_ff, ratio, ks, act, selector):
    """(parameters, x, fp64 y, periods) of one shape: computed once, shared by engines and alignments."""
    wide = C >= WIDE
    P = _params(C, d_ff, ratio, ks, act)
    if selector == "native":
        n = NATIVE[wide]
        x = torch.from_numpy(_ftn().synth.make_input(n["B"], n["L"], C, seed=n["seed"], planted=n["planted"]))
        y, periods = oracle_fp64(x, P, act, n["K"], n["L"], ks=KSETS[ks])
    else:
        s = _stub(C, selector)
        x = torch.from_numpy(_ftn().synth.make_input(s["B"], s["L"], C, seed=s["seed"], planted=()))
        y, periods = oracle_fp64(x, P, act, 0, s["L"], s["periods"], _stub_amps(s), ks=KSETS[ks])
    return P, x, y, periods


def _block(ftn, C, d_ff, ratio, ks, engine, act, dev):
    blk = ftn.models.timesnet.TimesBlock(C, KSETS[ks], 0.0, act, d_ff=d_ff, bottleneck_ratio=ratio)
    blk.engine = engine
    blk.inception.load_state_dict(_params(C, d_ff, ratio, ks, act), strict=True)
    return blk.eval().to(dev)


def _strip(forms):
    return {k: v for k, v in forms.items() if k != "spectrum"}


@pytest.mark.gpu
@pytest.mark.parametrize("selector", SELECTORS)
@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("C,d_ff,ratio,ks,engine", SMALL_BASE)
def test_small_forms_match_fp64_oracle(C, d_ff, ratio, ks, engine, act, align, selector, ftn):
    dev = torch.device("cuda:0")
    P, x, y_ref, periods = _reference(C, d_ff, ratio, ks, act, selector)
    T = ftn.models.timesnet
    blk = _block(ftn, C, d_ff, ratio, ks, engine, act, dev)
    B, L, _ = x.shape
    if selector == "native":
        blk.period_selector = T.FFTPeriodSelector(NATIVE[C >= WIDE]["K"], L)
    else:
        object.__setattr__(blk, "period_selector", _Stub(periods, _stub_amps(_stub(C, selector))))
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
    want = expected_forms_small(C, d_ff, ratio, ks, engine, act, 0, align == "aligned", fused)
    assert _strip(forms) == want
    assert _strip(forms_ln) == want
    if selector == "native":
        assert blk.period_selector.last_selected_periods.tolist() == periods
        assert forms["spectrum"] == ftn.runtime.spectrum_form(B, L, C, xd.data_ptr() % 16)
    assert blk._last_group_count == len(orc.period_group(periods, L, 1, L).periods)
    err = _check(y, y_ref, engine, RTOL, ATOL)
    ln_ref = torch.nn.functional.layer_norm(y_ref, (C,), ln.weight.detach().double().cpu(), ln.bias.detach().double().cpu(),
                                            ln.eps)
    err_ln = _check(y_ln, ln_ref, engine, LN_RTOL, LN_ATOL)
    print(f"forms_small C={C} d_ff={d_ff} ratio={ratio} {ks} {engine} {act} {align} {selector}: {want['conv']} "
          f"{want['C']} {want['E']} max|y-y64|={err:.3e} ln {err_ln:.3e}")


@pytest.mark.gpu
@pytest.mark.parametrize("C,d_ff,ratio,ks,engine", TILED_ROWS)
def test_small_forms_multi_tile_grids(C, d_ff, ratio, ks, engine, ftn):
    """The same criterion on the ``STUB_TILED`` grids: every group's tile list has more than one tile."""
    s = STUB_TILED
    dh = ftn.lib.desc_from_periods(s["periods"], s["L"], 1, s["L"])
    assert [int(dh.g_ntx[g]) * int(dh.g_nty[g]) for g in range(int(dh.n_groups))] == [2, 2, 3]   # periods 3, 16, 399
    test_small_forms_match_fp64_oracle(C, d_ff, ratio, ks, engine, "gelu", "aligned", "tiled", ftn)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("C,d_ff,ratio,ks,engine", SMALL_HALF)
def test_small_forms_half_input(C, d_ff, ratio, ks, engine, dtype, ftn):
    """The forms only a half input reaches (stage E without k_out_h, the pixel-major stage C where fp32 inputs go
    position-major): the criterion of ``test_half_precision_input_roundtrip``, against the same block on fp32 x."""
    dev = torch.device("cuda:0")
    n = NATIVE[C >= WIDE]
    blk = _block(ftn, C, d_ff, ratio, ks, engine, "gelu", dev)
    blk.period_selector = ftn.models.timesnet.FFTPeriodSelector(n["K"], n["L"])
    x = torch.from_numpy(ftn.synth.make_input(n["B"], n["L"], C, seed=n["seed"], planted=n["planted"])).to(dev)
    with torch.inference_mode():
        y32 = blk(x)
        y16 = blk(x.to(dtype))
        forms = blk._last_forms
    assert blk._last_backend == "hip" and y16.dtype == dtype
    adt = ftn.runtime.ACT_DTYPE[dtype]
    want = expected_forms_small(C, d_ff, ratio, ks, engine, "gelu", adt, True, ftn.runtime.fuse_stage_a(blk._pack[1]))
    assert _strip(forms) == want
    np.testing.assert_allclose(y16.float().cpu().numpy(), y32.cpu().numpy(), rtol=0.05, atol=0.1)
    print(f"forms_small C={C} d_ff={d_ff} ratio={ratio} {ks} {engine} gelu {dtype} native: {want['conv']} {want['C']} "
          f"{want['E']} max|y16-y32|={float((y16.float() - y32).abs().max()):.3e}")


# ---- a y that is not 16-byte aligned: the scalar stores of stages E + F (yvec = False), which no module-level call
#      produces (runtime.timesblock_forward allocates y itself)
SENTINEL = -12345.0


@pytest.mark.gpu
@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("C,d_ff,ratio,ks,engine,stage_e", [
    (64, 256, 4.0, "k357", "f16x2", "k_out_h<2>"), (24, 96, 4.0, "k357", "f32", "k_out_fast"),
    (16, 16, 1.0, "k3", "f32", "k_out_merged"),
    (128, 512, 4.0, "k357", "f32", "k_out"),                     # LayerNorm as the separate in-place row pass over y
])
def test_misaligned_y_equals_aligned(C, d_ff, ratio, ks, engine, stage_e, norm, ftn):
    dev = torch.device("cuda:0")
    lib, rt = ftn.lib.load(), ftn.runtime
    B, L, periods = 3, 50, [49, 7, 16]
    blk = _block(ftn, C, d_ff, ratio, ks, engine, "gelu", dev)
    wblob, plan = blk._packed(dev)
    assert rt.timesblock_forms(plan, B, L, 0, 0)["E"] == stage_e
    x = torch.from_numpy(ftn.synth.make_input(B, L, C, seed=55, planted=())).to(dev)
    dh = ftn.lib.desc_from_periods(periods, L, 1, L)
    assert int(dh.n_groups) == 3
    w = torch.softmax(torch.from_numpy(np.random.RandomState(55).standard_normal(size=(B, 3)).astype(np.float32)), 1)
    sel = rt.selection_from_host(dh, w, dev)
    gamma, beta = torch.linspace(0.5, 1.5, C, device=dev), torch.linspace(-0.2, 0.2, C, device=dev)
    n = x.numel()

    def run(y):
        need = lib.ftn_timesblock_workspace_bytes(ctypes.byref(plan), B, L, sel.max_groups, sel.px_bound)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        st = torch.cuda.current_stream().cuda_stream
        if norm:
            rc = lib.ftn_timesblock_forward_norm(x.data_ptr(), y.data_ptr(), B, L, ctypes.byref(plan), wblob.data_ptr(),
                                                 sel.desc.data_ptr(), sel.weights.data_ptr(), sel.max_groups, sel.px_bound,
                                                 0, gamma.data_ptr(), beta.data_ptr(), 1e-5, ws.data_ptr(), ws.numel(), st, None)
        else:
            rc = lib.ftn_timesblock_forward(x.data_ptr(), y.data_ptr(), B, L, ctypes.byref(plan), wblob.data_ptr(),
                                            sel.desc.data_ptr(), sel.weights.data_ptr(), sel.max_groups, sel.px_bound, 0, 0,
                                            ws.data_ptr(), ws.numel(), st, None)
        ftn.lib.check(rc, "ftn_timesblock_forward")
        torch.cuda.synchronize()

    y_al = torch.full_like(x, SENTINEL)
    assert y_al.data_ptr() % 16 == 0
    run(y_al)
    buf = torch.full((n + 8,), SENTINEL, dtype=torch.float32, device=dev)
    y_mis = buf[1:1 + n].view(B, L, C)
    assert y_mis.is_contiguous() and y_mis.data_ptr() % 16 == 4
    run(y_mis)
    assert not bool((y_al == SENTINEL).any())                    # every element was written
    assert torch.equal(y_mis, y_al)                              # bit for bit
    assert float(buf[0]) == SENTINEL and bool((buf[1 + n:] == SENTINEL).all())
