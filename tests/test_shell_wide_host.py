"""The host side of the model shell at 128 < d_model <= 512 (``ftn_*_wide_*``: entries in csrc/shell_api.hip, form
rules in csrc/shell_wide.hip and csrc/timeproj.hip): exports, the form rules restated and compared over a table, every
argument error reported with the entry's name before anything touches a device, the width rule of ``models/shell.py``
and its ``FTN_SHELL_WIDE`` switch.  No GPU needed."""
import itertools
import os
import subprocess
import sys
import textwrap

import pytest

from conftest import ROOT

WIDE = ("ftn_embed_wide_forward", "ftn_embed_wide_rows_strided", "ftn_embed_wide_ring", "ftn_timeproj_wide_forward",
        "ftn_head_wide_forward", "ftn_embed_wide_form", "ftn_head_wide_form", "ftn_timeproj_wide_form")
DS, NS, STRIDES, MISALIGN = (132, 192, 256, 260, 512), (1, 5, 8, 64, 512), (0, 512, 513), (0, 4)


def test_exports_and_abi_version(ftn):
    lib = ftn.lib.load()
    assert lib.ftn_abi_version() == 14 and ftn.lib.ABI_VERSION == 14
    assert set(WIDE) <= set(ftn.lib.EXPORTS)
    for name in WIDE:
        assert hasattr(lib, name)


# ------------------------------------------------------------------------------------------------------------ forms
def embed_wide_rule(N, D, x_bs, x_mis, w_mis):
    """``embed_wide_form`` restated: 64-column slabs a wave up to d_model 256 and 128-column slabs beyond, 64 rows a
    workgroup; 16-byte loads need whole quads everywhere; the arithmetic is bf16x3 either way."""
    vec = N % 4 == 0 and x_bs % 4 == 0 and x_mis == 0 and w_mis == 0
    return f"k_embed_wide_bf<{4 if D <= 256 else 8},4,{'true' if vec else 'false'}>"


def head_wide_rule(N, D, tail_bs, late_bs, mis):
    """``head_wide_form`` restated, with the cap on ``gridDim.y``: as many workgroups a CU as 160 KB of LDS hold."""
    if not (N % 4 == 0 and tail_bs % 4 == 0 and late_bs % 4 == 0 and mis == 0):
        return "k_head_wide_f32", 0
    nt = 2 if D <= 256 else 1
    lds = 2 * nt * -(-D // 32) * 3 * 1024 + 3 * 16 * nt * 4
    ntile = -(-N // (16 * nt))
    return f"k_head_wide_bf<{nt}>", -(-(160 * 1024 // lds) * 256 // ntile)


def timeproj_wide_rule(L, S, D, mis):
    if S == 1:
        return "k_timeproj_row_wide"
    tiles = -(-S // 16)
    nst = 1 if tiles <= 1 else 2 if tiles <= 2 else 4 if tiles <= 4 else 6
    return f"k_timeproj_bf<{nst},{'true' if L % 4 == 0 and mis == 0 else 'false'}>"


def test_embed_forms_over_the_table(ftn):
    rt, seen = ftn.runtime, set()
    for N, D, bs, xm, wm in itertools.product(NS, DS, STRIDES, MISALIGN, MISALIGN):
        got = rt.embed_wide_form_of(N, D, bs, xm, wm)
        assert got == embed_wide_rule(N, D, bs, xm, wm) == rt.embed_form_at(N, D, bs, xm, wm), (N, D, bs, xm, wm)
        seen.add(got)
    assert seen == {f"k_embed_wide_bf<{no},4,{vec}>" for no in (4, 8) for vec in ("true", "false")}
    lib = ftn.lib.load()
    assert lib.ftn_embed_wide_form(64, 132, 0, 0, 0) == 1 | 2 | 4 << 4 | 4 << 8        # BF, VEC, NO 4, RT 4
    assert lib.ftn_embed_wide_form(64, 256, 0, 0, 0) == 1 | 2 | 4 << 4 | 4 << 8
    assert lib.ftn_embed_wide_form(64, 260, 0, 0, 0) == 1 | 2 | 8 << 4 | 4 << 8
    assert lib.ftn_embed_wide_form(5, 512, 0, 0, 0) == 1 | 8 << 4 | 4 << 8


def test_head_forms_over_the_table(ftn):
    rt, seen = ftn.runtime, set()
    for N, D, tbs, lbs, mis in itertools.product(NS, DS, STRIDES, (0, 4, 513), MISALIGN + (12,)):
        got = rt.head_wide_form_of(N, D, tbs, lbs, mis)
        assert got == head_wide_rule(N, D, tbs, lbs, mis) == rt.head_form_at(N, D, tbs, lbs, mis), (N, D, tbs, lbs, mis)
        seen.add(got[0])
    assert seen == {"k_head_wide_f32", "k_head_wide_bf<2>", "k_head_wide_bf<1>"}
    assert rt.head_wide_form_of(64, 256) == ("k_head_wide_bf<2>", 128)      # 96 KB: one workgroup a CU, two series tiles
    assert rt.head_wide_form_of(64, 512) == ("k_head_wide_bf<1>", 64)


def test_timeproj_forms_over_the_table(ftn):
    rt, seen = ftn.runtime, set()
    for L, S, D, mis in itertools.product((1, 5, 33, 96, 336), (1, 2, 17, 64, 96, 100), DS, (0, 4, 8, 12)):
        got = rt.timeproj_wide_form_of(L, S, D, mis)
        assert got == timeproj_wide_rule(L, S, D, mis) == rt.timeproj_form_at(L, S, D, mis), (L, S, D, mis)
        seen.add(got)
    assert seen == {"k_timeproj_row_wide"} | {f"k_timeproj_bf<{n},{w}>" for n in (1, 2, 4, 6) for w in ("true", "false")}


def test_narrow_queries_keep_their_limit_and_the_dispatch_follows_d_model(ftn):
    rt = ftn.runtime
    assert rt.embed_form_at(64, 128) == rt.embed_form_of(64, 128) == "k_embed_in_bf<8,1>"
    assert rt.head_form_at(64, 128) == rt.head_form_of(64, 128) and rt.timeproj_form_at(24, 1, 128) == "k_timeproj_row"
    for fn, args, name in ((rt.embed_form_of, (8, 132), "ftn_embed_form"), (rt.head_form_of, (8, 132), "ftn_head_form"),
                           (rt.timeproj_form_of, (24, 4, 132), "ftn_timeproj_form")):
        with pytest.raises(ValueError, match=name):
            fn(*args)


@pytest.mark.parametrize("D", [128, 130, 516, 0, -4])
def test_form_queries_reject_d_model_outside_the_wide_range(D, ftn):
    rt = ftn.runtime
    for fn, args, name in ((rt.embed_wide_form_of, (8, D), "ftn_embed_wide_form"),
                           (rt.head_wide_form_of, (8, D), "ftn_head_wide_form"),
                           (rt.timeproj_wide_form_of, (24, 4, D), "ftn_timeproj_wide_form")):
        with pytest.raises(ValueError, match=name):
            fn(*args)


def test_form_queries_reject_bad_arguments(ftn):
    rt = ftn.runtime
    for args in [(0, 256, 0, 0, 0), (8, 256, 0, 3, 0), (8, 256, 0, 16, 0), (8, 256, 0, 0, -4)]:
        with pytest.raises(ValueError, match="ftn_embed_wide_form"):
            rt.embed_wide_form_of(*args)
    for args in [(0, 256, 0, 0, 0), (8, 256, 0, 0, 5), (8, 256, 0, 0, 16)]:
        with pytest.raises(ValueError, match="ftn_head_wide_form"):
            rt.head_wide_form_of(*args)
    for args in [(0, 4, 256, 0), (24, 0, 256, 0), (24, 4, 256, 2), (24, 4, 256, 16)]:
        with pytest.raises(ValueError, match="ftn_timeproj_wide_form"):
            rt.timeproj_wide_form_of(*args)


# ---------------------------------------------------------------------------------------- argument checks of the entries
A, M = 0x10000, 0x10004          # stand-ins for device addresses: 16-byte aligned / 4 bytes past a boundary
BAD_D = {"D = 128": dict(D=128), "D = 130": dict(D=130), "D = 516": dict(D=516), "D = 0": dict(D=0)}


def _embed_forward(lib, a):
    return lib.ftn_embed_wide_forward(a["x"], a["x_bs"], a["B"], a["L"], a["N"], a["w"], a["D"], a["add"], a["add_bs"],
                                      a["g"], a["b"], 1e-5, a["out"], None)


def _embed_rows(lib, a):
    return lib.ftn_embed_wide_rows_strided(a["x"], a["x_bs"], a["B"], a["L"], a["N"], a["w"], a["D"], a["out"],
                                           a["out_bs"], None)


def _embed_ring(lib, a):
    return lib.ftn_embed_wide_ring(a["V"], a["B"], a["L"], a["D"], a["head"], a["add"], a["add_bs"], a["g"], a["b"],
                                   1e-5, a["out"], None)


def _timeproj(lib, a):
    return lib.ftn_timeproj_wide_forward(a["seq"], a["B"], a["L"], a["D"], a["wt"], a["bt"], a["S"], a["hid"], None)


def _head(lib, a):
    return lib.ftn_head_wide_forward(a["hidden"], a["rows"], a["S"], a["D"], a["N"], a["wmu"], a["bmu"], a["wsg"],
                                     a["bsg"], a["tail"], 0, a["hist"], a["late"], 0, None, 1e-3, a["rate"], a["disp"],
                                     a["bad"], None)


ENTRIES = {
    "ftn_embed_wide_forward": (_embed_forward, dict(x=A, x_bs=24 * 8, B=2, L=24, N=8, w=A, D=256, add=A, add_bs=0, g=A,
                                                     b=A, out=A), {
        **BAD_D, "null x": dict(x=None), "null W": dict(w=None), "null out": dict(out=None), "B = 0": dict(B=0),
        "L = 0": dict(L=0), "N = 0": dict(N=0), "out misaligned": dict(out=M), "add misaligned": dict(add=M),
        "gamma without beta": dict(b=None), "add stride": dict(add_bs=6)}),
    "ftn_embed_wide_rows_strided": (_embed_rows, dict(x=A, x_bs=24 * 8, B=2, L=24, N=8, w=A, D=256, out=A,
                                                       out_bs=24 * 256), {
        **BAD_D, "null x": dict(x=None), "null W": dict(w=None), "null out": dict(out=None), "B = 0": dict(B=0),
        "out misaligned": dict(out=M), "out off by 8": dict(out=A + 8), "rows overlap": dict(out_bs=23 * 256),
        "out stride": dict(out_bs=24 * 256 + 2)}),
    "ftn_embed_wide_ring": (_embed_ring, dict(V=A, B=2, L=24, D=256, head=3, add=A, add_bs=0, g=A, b=A, out=A), {
        **BAD_D, "null V": dict(V=None), "null out": dict(out=None), "L = 0": dict(L=0), "head = L": dict(head=24),
        "head < 0": dict(head=-1), "V misaligned": dict(V=M), "out misaligned": dict(out=M),
        "beta without gamma": dict(g=None)}),
    "ftn_timeproj_wide_forward": (_timeproj, dict(seq=A, B=2, L=24, D=256, wt=A, bt=A, S=4, hid=A), {
        **BAD_D, "null seq": dict(seq=None), "null wt": dict(wt=None), "null bt": dict(bt=None),
        "null hidden": dict(hid=None), "B = 0": dict(B=0), "L = 0": dict(L=0), "S = 0": dict(S=0),
        "seq misaligned": dict(seq=M), "hidden misaligned": dict(hid=M), "hidden off by 8": dict(hid=A + 8)}),
    "ftn_head_wide_forward": (_head, dict(hidden=A, rows=12, S=4, D=256, N=8, wmu=A, bmu=A, wsg=A, bsg=A, tail=A, hist=4,
                                          late=None, rate=A, disp=A, bad=A), {
        **BAD_D, "null hidden": dict(hidden=None), "null w_mu": dict(wmu=None), "null b_sigma": dict(bsg=None),
        "null tail": dict(tail=None), "null rate": dict(rate=None), "null disp": dict(disp=None),
        "null flag": dict(bad=None), "rows % S": dict(rows=13), "rows = 0": dict(rows=0), "hist > S": dict(hist=5),
        "hist = 0": dict(hist=0), "N = 0": dict(N=0), "hidden misaligned": dict(hidden=M),
        "w_sigma misaligned": dict(wsg=M)}),
}
CASES = [(entry, name) for entry, (_, _, bad) in ENTRIES.items() for name in bad]


@pytest.mark.parametrize("entry,name", CASES, ids=[f"{e[4:]}-{n}" for e, n in CASES])
def test_entries_reject_bad_arguments_before_any_launch(entry, name, ftn):
    """None of these reaches a launch (this test runs without a device): non-zero return, and the last error starts
    with the entry's name."""
    lib = ftn.lib.load()
    call, good, bad = ENTRIES[entry]
    assert lib.ftn_timeproj_wide_form(24, 4, 256, 0) > 0                 # leaves an earlier message out of the way
    rc = call(lib, {**good, **bad[name]})
    assert rc != 0
    msg = lib.ftn_last_error().decode()
    assert msg.startswith(entry + ":"), msg
    with pytest.raises(ValueError, match=entry):
        ftn.lib.check(rc, entry)


def test_the_narrow_entries_still_reject_132(ftn):
    lib = ftn.lib.load()
    assert lib.ftn_embed_forward(A, 0, 1, 4, 8, A, 132, None, 0, None, None, 0.0, A, None) != 0
    assert lib.ftn_last_error().decode().startswith("ftn_embed_forward")
    assert lib.ftn_timeproj_forward(A, 2, 24, 132, A, A, 4, A, None) != 0
    assert lib.ftn_last_error().decode().startswith("ftn_timeproj_forward")
    assert lib.ftn_embed_ring(A, 2, 24, 132, 0, None, 0, None, None, 0.0, A, None) != 0
    assert lib.ftn_last_error().decode().startswith("ftn_embed_ring")


# --------------------------------------------------------------------------------------------------- the width rule
def test_width_rules(ftn):
    sh = ftn.models.shell
    assert all(sh.hip_shell_width_ok(d) for d in (4, 128, 132, 512))
    assert not sh.hip_shell_width_ok(130) and not sh.hip_shell_width_ok(516)
    assert sh.hip_width_ok(128) and not sh.hip_width_ok(132)


_PROBE = textwrap.dedent("""
    import sys
    sys.path.insert(0, {root!r})
    import torch
    import __graft_entry__ as ge
    ftn = ge.load_package()

    class DeviceWindow:                    # what _hip_embed_ok reads of a contiguous fp32 [2, 8, 6] window on a device
        is_cuda, dtype, requires_grad = True, torch.float32, False
        def stride(self, i): return (48, 6, 1)[i]
        def size(self, i): return (2, 8, 6)[i]

    out = []
    for d_model in (128, 192):
        net = ftn.models.TimesNet(input_len=8, pred_len=2, d_model=d_model, n_layers=1, k_periods=1,
                                  kernel_set=[(3, 3)], dropout=0.0, activation="gelu", mode="direct").eval()
        with torch.inference_mode():
            net(torch.rand(2, 8, 6) + 1.0)
            out.append(int(net._hip_embed_ok(DeviceWindow())))
    print("EMBED_OK", *out, int(ftn.models.shell.hip_shell_width_ok(192)))
""")


@pytest.mark.parametrize("value,want", [(None, "EMBED_OK 1 1 1"), ("1", "EMBED_OK 1 1 1"), ("0", "EMBED_OK 1 0 0")])
def test_shell_wide_switch_restores_the_torch_shell(value, want):
    """``FTN_SHELL_WIDE=0`` (read once per process): ``_hip_embed_ok`` is false at d_model 192 and still true at 128."""
    env = {k: v for k, v in os.environ.items() if k != "FTN_SHELL_WIDE"}
    if value is not None:
        env["FTN_SHELL_WIDE"] = value
    r = subprocess.run([sys.executable, "-c", _PROBE.format(root=str(ROOT))], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip().splitlines()[-1] == want
