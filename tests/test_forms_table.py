"""The dispatch table of the block's kernel forms (``ftn_timesblock_forms``, host-only: no GPU needed), pinned for
the d_model 64 / 128 pipeline shapes at every parameter tuple the GPU form tests (``test_gpu_forms.py``) run, under
the switches that select replacement forms, and across window lengths."""
import os
import subprocess
import sys
import textwrap

import pytest

from conftest import ROOT
from test_gpu_forms import (FORMS_MATRIX, KS, NATIVE, STUB, TABLE_FORMS, WIDTHS, expected_forms)


def _plan(ftn, C, engine, act):
    sd = ftn.synth.make_inception_params(C, 4 * C, KS, 4.0, seed=0)
    return ftn.pack.pack_inception(sd, C, 4 * C, KS, 4.0, act, engine)[1]


@pytest.mark.parametrize("L", [NATIVE["L"], STUB["L"]])
def test_forms_of_every_gpu_case(L, ftn):
    seen = set()
    for C, engine, act, adt, aligned in FORMS_MATRIX:
        plan = _plan(ftn, C, engine, act)
        got = ftn.runtime.timesblock_forms(plan, 3, L, adt, 0 if aligned else 4)
        assert got == expected_forms(C, engine, act, adt, aligned), (C, engine, act, adt, aligned)
        seen.add((got["conv"], got["C"], got["E"], got["act"], got["xvec"]))
    # every row of the table is returned for both activations (and, for fp32 inputs, both alignments): a dispatch
    # change that stops producing a form fails here, not silently in the GPU suite
    for (C, engine, inp), forms in TABLE_FORMS.items():
        for act in ("gelu", "relu"):
            for xvec in ((True, False) if inp != "half" else (True,)):
                assert forms + (act, xvec) in seen, (C, engine, inp, act, xvec)


def test_fast_conv_over_window_lengths(ftn):
    """The fast conv forms hold at every window length tried: the clipped conv region never exceeds FTN_REGION_PX
    for the 3x3 / 5x5 / 7x7 kernel set (``ftn_tile_geometry`` shrinks the tiles), so no supported L drops them."""
    plans = {C: _plan(ftn, C, "f16x2", "gelu") for C in WIDTHS}
    for L in [2, 3, 7, 16, 33, 96, 97, 150, 250, 336, 512, 720, 1023, 2100, 4096]:
        assert ftn.runtime.timesblock_forms(plans[64], 1, L)["conv"] == "k_conv_bf_fast<2,1>", L
        assert ftn.runtime.timesblock_forms(plans[128], 1, L)["conv"] == "k_conv_bf_fast<2,2>", L


def test_forms_query_rejects_bad_arguments(ftn):
    plan = _plan(ftn, 64, "f16x2", "gelu")
    for args in [(0, 336, 0, 0), (1, 1, 0, 0), (1, 336, 3, 0), (1, 336, 0, 16)]:
        with pytest.raises(ValueError, match="ftn_timesblock_forms"):
            ftn.runtime.timesblock_forms(plan, *args)
    with pytest.raises(ValueError, match="ftn_period_spectrum_form"):
        ftn.runtime.spectrum_form(0, 336, 64)


def test_spectrum_forms(ftn):
    f = ftn.runtime.spectrum_form
    assert f(3, 336, 64) == ("k_spectrum", False) == f(3, 336, 64, 4)
    assert f(64, 336, 64) == ("k_spectrum_rowq", True) and f(64, 336, 64, 4) == ("k_spectrum_rowq", False)
    assert f(64, 250, 64) == ("k_spectrum_row", True) and f(64, 250, 64, 8) == ("k_spectrum_row", False)
    assert f(3, 336, 128) == ("k_spectrum_rowq_tiled", True) and f(3, 336, 128, 4) == ("k_spectrum_rowq_tiled", False)
    assert f(3, 336, 128, 0, scratch=False) == ("k_spectrum", False)
    assert f(64, 336, 62) == ("k_spectrum_rowq", False)          # C % 4 != 0: scalar loads


_PROBE = textwrap.dedent("""
    import json, sys
    sys.path.insert(0, {root!r})
    import __graft_entry__ as ge
    ftn = ge.load_package()
    ks = [(3, 3), (5, 5), (7, 7)]
    out = {{}}
    for C in (64, 128):
        sd = ftn.synth.make_inception_params(C, 4 * C, ks, 4.0, seed=0)
        plan = ftn.pack.pack_inception(sd, C, 4 * C, ks, 4.0, "relu", "f16x2")[1]
        out[C] = ftn.runtime.timesblock_forms(plan, 3, 336)
    print(json.dumps(out))
""")


@pytest.mark.parametrize("switch,want64,want128", [
    # stage C falls back to the unit-per-wave kernel, R keeping x; k_out_h stays
    ("FTN_MLP_POS=0", ("k_mlp_bf_u1<2>", True, False, "k_out_h<2>"), ("k_mlp_bf_c128<2>", False, False, "k_out_h<2>")),
    # fp32 stage E: at d_model 64 the FAST k_out reads the group-summed R; at 128 k_mlp_pos128 needs k_out_h
    ("FTN_OUT_H=0", ("k_mlp_pos64<2>", True, True, "k_out_fast"), ("k_mlp_bf_c128<2>", False, False, "k_out")),
    ("FTN_MLP_U1=0", ("k_mlp_bf<2>", False, False, "k_out_h<2>"), ("k_mlp_bf_c128<2>", False, False, "k_out_h<2>")),
    ("FTN_R_KEEPS_X=0", ("k_mlp_pos64<2>", True, True, "k_out_h<2>"), ("k_mlp_pos128<2>", True, True, "k_out_h<2>")),
])
def test_switches_select_replacement_forms(switch, want64, want128):
    name, value = switch.split("=")
    r = subprocess.run([sys.executable, "-c", _PROBE.format(root=str(ROOT))], env=dict(os.environ, **{name: value}),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    import json
    got = json.loads(r.stdout.strip().splitlines()[-1])
    for C, want in (("64", want64), ("128", want128)):
        f = got[C]
        assert (f["C"], f["r_keeps_x"], f["r_summed"], f["E"]) == want, (switch, C, f)
        assert f["act"] == "relu"


def test_conv_generic_switch_drops_fast_conv():
    r = subprocess.run([sys.executable, "-c", _PROBE.format(root=str(ROOT))], env=dict(os.environ, FTN_CONV_GENERIC="1"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    import json
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got["64"]["conv"] == "k_conv_bf<1,2>" and got["128"]["conv"] == "k_conv_bf<2,2>", got
