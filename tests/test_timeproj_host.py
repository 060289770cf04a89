"""The time projection's host side (``ftn_timeproj_form``, the argument checks of ``ftn_timeproj_forward``): no GPU
needed.  The form rule is restated here and compared over a table; every argument error must be reported, with a
message, before anything touches a device."""
import itertools

import pytest


def form_rule(L, S, D, misalign):
    """``timeproj_form`` (csrc/timeproj.hip) restated: the row form for one output step; otherwise bf16x3 with NST =
    the smallest of 1, 2, 4, 6 tiles of 16 steps that covers S (6 beyond 96 steps, where the grid walks chunks) and
    16-byte loads of W_t when its rows allow them."""
    if S == 1:
        return "k_timeproj_row"
    tiles = -(-S // 16)
    nst = 1 if tiles <= 1 else 2 if tiles <= 2 else 4 if tiles <= 4 else 6
    return f"k_timeproj_bf<{nst},{'true' if L % 4 == 0 and misalign == 0 else 'false'}>"


TABLE = list(itertools.product((1, 5, 31, 32, 33, 96, 336, 720), (1, 2, 15, 16, 17, 32, 33, 64, 65, 96, 97, 200),
                               (4, 12, 36, 64, 68, 128), (0, 4, 8, 12)))


def test_form_rule_over_the_table(ftn):
    rt = ftn.runtime
    seen = set()
    for L, S, D, mis in TABLE:
        got = rt.timeproj_form_of(L, S, D, mis)
        assert got == form_rule(L, S, D, mis), (L, S, D, mis, got)
        seen.add(got)
    assert seen == {"k_timeproj_row"} | {f"k_timeproj_bf<{n},{w}>" for n in (1, 2, 4, 6) for w in ("true", "false")}, seen


def test_form_encoding(ftn):
    """The raw value: bit 0 the 16-bit form, bit 1 vector loads of W_t, NST in bits 4-7, eight waves in bits 8-11."""
    lib = ftn.lib.load()
    assert lib.ftn_timeproj_form(336, 1, 64, 0) == 0 and lib.ftn_timeproj_form(335, 1, 64, 12) == 0
    assert lib.ftn_timeproj_form(336, 96, 64, 0) == 1 | 2 | 6 << 4 | 8 << 8
    assert lib.ftn_timeproj_form(335, 96, 64, 0) == 1 | 6 << 4 | 8 << 8
    assert lib.ftn_timeproj_form(336, 17, 128, 4) == 1 | 2 << 4 | 8 << 8


@pytest.mark.parametrize("args", [(0, 4, 64, 0), (24, 0, 64, 0), (24, 4, 0, 0), (24, 4, 66, 0), (24, 4, 132, 0),
                                  (24, 4, 64, 2), (24, 4, 64, 16), (24, 4, 64, -4)])
def test_form_rejects_bad_arguments(args, ftn):
    lib = ftn.lib.load()
    assert lib.ftn_timeproj_form(*args) < 0
    assert b"ftn_timeproj_form" in lib.ftn_last_error()
    with pytest.raises(ValueError, match="ftn_timeproj_form"):
        ftn.runtime.timeproj_form_of(*args)


A, M = 0x10000, 0x10004          # stand-ins for device addresses: 16-byte aligned / 4 bytes past a boundary
GOOD = dict(seq=A, B=2, L=24, D=64, wt=A, bt=A, S=4, hid=A)
BAD = {
    "null seq": dict(seq=None), "null wt": dict(wt=None), "null bt": dict(bt=None), "null hidden": dict(hid=None),
    "B = 0": dict(B=0), "L = 0": dict(L=0), "S = 0": dict(S=0), "B < 0": dict(B=-3),
    "D % 4": dict(D=66), "D = 0": dict(D=0), "D > 128": dict(D=132),
    "seq misaligned": dict(seq=M), "hidden misaligned": dict(hid=M), "hidden off by 8": dict(hid=A + 8),
}


@pytest.mark.parametrize("name", list(BAD))
def test_forward_rejects_bad_arguments_before_any_launch(name, ftn):
    """None of these reaches a launch (this test runs without a device): non-zero return, and the last error names
    the entry point."""
    lib = ftn.lib.load()
    a = {**GOOD, **BAD[name]}
    assert lib.ftn_timeproj_form(24, 4, 64, 0) > 0                      # leaves an earlier message out of the way
    rc = lib.ftn_timeproj_forward(a["seq"], a["B"], a["L"], a["D"], a["wt"], a["bt"], a["S"], a["hid"], None)
    assert rc != 0
    msg = lib.ftn_last_error().decode()
    assert msg.startswith("ftn_timeproj_forward"), msg
    with pytest.raises(ValueError, match="ftn_timeproj_forward"):
        ftn.lib.check(rc, "ftn_timeproj_forward")


def test_misaligned_weight_slice_is_not_an_error(ftn):
    """W_t = weight[-S:] at L % 4 != 0 starts 4 bytes past a boundary: a form, not an error."""
    assert ftn.runtime.timeproj_form_of(25, 4, 64, 4) == "k_timeproj_bf<1,false>"
    assert ftn.runtime.timeproj_form_of(25, 1, 64, 4) == "k_timeproj_row"


def test_abi_version_and_exports(ftn):
    lib = ftn.lib.load()
    assert lib.ftn_abi_version() == 14 and ftn.lib.ABI_VERSION == 14
    assert {"ftn_timeproj_forward", "ftn_timeproj_form"} <= set(ftn.lib.EXPORTS)


def test_wrapper_validates_layout_on_the_host(ftn):
    import torch

    rt = ftn.runtime
    seq, wt, bt = torch.zeros(2, 24, 64), torch.zeros(4, 24), torch.zeros(4)
    with pytest.raises(ValueError, match="device"):
        rt.timeproj_forward(seq, wt, bt)
    with pytest.raises(ValueError, match="project"):
        rt.timeproj_forward(seq, torch.zeros(4, 23), bt)
    with pytest.raises(ValueError, match="seq \\[B, L, D\\]"):
        rt.timeproj_forward(seq[0], wt, bt)
