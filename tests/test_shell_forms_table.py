"""The dispatch table of the model-shell kernels (``ftn_embed_form``, ``ftn_head_form``; host-only, no GPU needed):
the reported form equals an independent restatement of the rule over a grid of shapes, strides and misalignments,
every form of ``csrc/shell.hip`` is returned by at least one grid point, and the environment switches
(``FTN_EMBED_F32``, ``FTN_EMBED_RT``, ``FTN_HEAD_F32``) are reflected (in subprocesses: the library reads them once)."""
import json
import os
import subprocess
import sys
import textwrap

import pytest

from conftest import ROOT

DS = list(range(4, 129, 4))
NS = list(range(1, 10)) + list(range(60, 69)) + [512]
STRIDES = [0, 1, 2, 4, 6, 512, 513]          # batch strides in elements (0: one batch row, or shared)
MISALIGN = [0, 4, 8]                         # bytes from a 16-byte boundary

# the eight + eleven forms of csrc/shell.hip: four + seven are reached from shape and alignment alone (the grid
# tests assert exactly that set), the other four + four only under a switch (the subprocess test asserts each)


def embed_rule(N, D, x_bs, x_mis, w_mis, f32=False, rt=0):
    """``embed_launch`` restated: the 16-bit form needs whole 16-byte quads everywhere."""
    no = 4 if D <= 64 else 8
    vec = N % 4 == 0 and x_bs % 4 == 0 and x_mis == 0 and w_mis == 0
    if vec and not f32:
        return f"k_embed_in_bf<{no},{rt if rt else (2 if no == 4 else 1)}>"
    return f"k_embed_in<{no},{'true' if vec else 'false'}>"


def head_rule(N, D, tail_bs, late_bs, mis, f32=False):
    """``ftn_head_forward`` restated, with the cap on ``gridDim.y``."""
    vec = N % 4 == 0 and tail_bs % 4 == 0 and late_bs % 4 == 0 and mis == 0
    if vec and not f32:
        nt, ns32 = (4, 1) if D <= 32 else (4, 2) if D <= 64 else (2, 4)
        ntile = -(-N // (16 * nt))
        return f"k_head_bf<{nt},{ns32}>", -(-768 // ntile)
    ns = 1 if D <= 16 else 2 if D <= 32 else 4 if D <= 64 else 8
    ntile = -(-N // 64)
    return f"k_head<{ns},{'true' if vec else 'false'}>", -(-1024 // ntile)


def _embed_grid():
    for D in DS:
        for N in NS:
            for bs in STRIDES:
                for xm in MISALIGN:
                    for wm in MISALIGN:
                        yield N, D, bs, xm, wm


def _head_grid():
    for D in DS:
        for N in NS:
            for tbs in STRIDES:
                for lbs in (0, 4, 513):
                    for mis in MISALIGN + [12]:
                        yield N, D, tbs, lbs, mis


def test_embed_forms_over_the_grid(ftn):
    rt, seen = ftn.runtime, set()
    for args in _embed_grid():
        got = rt.embed_form_of(*args)
        assert got == embed_rule(*args), args
        seen.add(got)
    # without switches the library never picks the fp32 vector forms or the non-default RT: those are pinned by the
    # switch tests below; everything else must be reachable from shape and alignment alone
    assert seen == {"k_embed_in<4,false>", "k_embed_in<8,false>", "k_embed_in_bf<4,2>", "k_embed_in_bf<8,1>"}, seen


def test_head_forms_over_the_grid(ftn):
    rt, seen = ftn.runtime, set()
    for args in _head_grid():
        got = rt.head_form_of(*args)
        assert got == head_rule(*args), args
        seen.add(got[0])
    assert seen == {f"k_head<{ns},false>" for ns in (1, 2, 4, 8)} | {"k_head_bf<4,1>", "k_head_bf<4,2>",
                                                                     "k_head_bf<2,4>"}, seen


def test_tensor_queries_follow_pointer_and_stride(ftn):
    """``embed_form`` / ``head_form`` read the tensors as ``embed_forward`` / ``head_forward`` pass them on (CPU
    tensors serve: only shape, stride and address are read)."""
    import torch

    rt = ftn.runtime
    big = torch.zeros(3 * 10 * 8 + 16)
    base = (-(big.data_ptr() // 4)) % 4                     # first 16-byte aligned element
    w64, w128 = torch.zeros(64, 8), torch.zeros(128, 8)
    assert w64.data_ptr() % 16 == 0 and w128.data_ptr() % 16 == 0
    aligned = big[base:base + 240].view(3, 10, 8)
    off1 = big[base + 1:base + 241].view(3, 10, 8)
    assert rt.embed_form(aligned, w64) == "k_embed_in_bf<4,2>" and rt.embed_form(aligned, w128) == "k_embed_in_bf<8,1>"
    assert rt.embed_form(off1, w64) == "k_embed_in<4,false>" and rt.embed_form(off1, w128) == "k_embed_in<8,false>"
    assert rt.embed_form(aligned[:, -4:], w64) == "k_embed_in_bf<4,2>"          # batch stride 80, offset 48 elements
    odd = big[base:base + 3 * 83].view(3, 83)[:, :80].unflatten(1, (10, 8))     # batch stride 83
    assert odd.stride() == (83, 8, 1) and rt.embed_form(odd, w64) == "k_embed_in<4,false>"
    assert rt.embed_form(odd[:1], w64) == "k_embed_in_bf<4,2>"                  # B = 1: the stride is passed as 0
    hidden, wmu = torch.zeros(3, 10, 16), torch.zeros(8, 16)
    assert rt.head_form(hidden, wmu, aligned) == ("k_head_bf<4,1>", 768)
    assert rt.head_form(hidden, wmu, off1) == ("k_head<1,false>", 1024)
    assert rt.head_form(hidden, wmu, odd) == ("k_head<1,false>", 1024)
    late = torch.zeros(3, 10, 8)
    assert rt.head_form(hidden, wmu, aligned, late) == ("k_head_bf<4,1>", 768)
    assert rt.head_form(hidden, wmu, aligned, off1) == ("k_head<1,false>", 1024)  # (a misaligned late bias)


def test_form_queries_reject_bad_arguments(ftn):
    rt = ftn.runtime
    for args in [(0, 64, 0, 0, 0), (8, 0, 0, 0, 0), (8, 6, 0, 0, 0), (8, 132, 0, 0, 0), (8, 64, 0, 3, 0),
                 (8, 64, 0, 16, 0), (8, 64, 0, 0, -4)]:
        with pytest.raises(ValueError, match="ftn_embed_form"):
            rt.embed_form_of(*args)
    for args in [(0, 64, 0, 0, 0), (8, 2, 0, 0, 0), (8, 130, 0, 0, 0), (8, 64, 0, 0, 5), (8, 64, 0, 0, 16)]:
        with pytest.raises(ValueError, match="ftn_head_form"):
            rt.head_form_of(*args)


_PROBE = textwrap.dedent("""
    import json, sys
    sys.path.insert(0, {root!r})
    import __graft_entry__ as ge
    rt = ge.load_package().runtime
    out = {{"embed": [], "head": []}}
    for D in (4, 16, 20, 32, 36, 64, 68, 128):
        for N in (5, 8, 64, 512):
            for bs in (0, 512, 513):
                for mis in (0, 4):
                    out["embed"].append([[N, D, bs, mis, 0], rt.embed_form_of(N, D, bs, mis, 0)])
                    out["embed"].append([[N, D, bs, 0, mis], rt.embed_form_of(N, D, bs, 0, mis)])
                    out["head"].append([[N, D, bs, 0, mis], list(rt.head_form_of(N, D, bs, 0, mis))])
                    out["head"].append([[N, D, 0, bs, mis], list(rt.head_form_of(N, D, 0, bs, mis))])
    print(json.dumps(out))
""")


@pytest.mark.parametrize("switch,new_forms", [
    ("FTN_EMBED_F32=1", {"k_embed_in<4,true>", "k_embed_in<8,true>"}),
    ("FTN_EMBED_RT=1", {"k_embed_in_bf<4,1>"}),
    ("FTN_EMBED_RT=2", {"k_embed_in_bf<8,2>"}),
    ("FTN_HEAD_F32=1", {f"k_head<{ns},true>" for ns in (1, 2, 4, 8)}),
])
def test_switches_select_the_other_forms(switch, new_forms):
    name, value = switch.split("=")
    env = {k: v for k, v in os.environ.items() if k not in ("FTN_EMBED_F32", "FTN_EMBED_RT", "FTN_HEAD_F32")}
    r = subprocess.run([sys.executable, "-c", _PROBE.format(root=str(ROOT))], env=dict(env, **{name: value}),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    kw_e = {"f32": name == "FTN_EMBED_F32", "rt": int(value) if name == "FTN_EMBED_RT" else 0}
    kw_h = {"f32": name == "FTN_HEAD_F32"}
    seen = set()
    for args, form in got["embed"]:
        assert form == embed_rule(*args, **kw_e), (switch, args)
        seen.add(form)
    for args, form in got["head"]:
        assert tuple(form) == head_rule(*args, **kw_h), (switch, args)
        seen.add(form[0])
    assert new_forms <= seen, (switch, new_forms - seen)

