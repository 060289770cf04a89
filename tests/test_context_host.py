"""The host side of the context front end (``ftn_context_rows``, ``ftn_context_through_weight``, ``ftn_embed_add``,
csrc/context.hip): exports, the form rules restated and compared over a table, every argument error reported with the
entry's name before anything touches a device, and the ``FTN_CTX_HIP`` switch of ``models/shell.py``.  No GPU needed."""
import ctypes as C
import itertools
import os
import subprocess
import sys
import textwrap

import pytest

from conftest import ROOT

ENTRY_NAMES = ("ftn_context_rows", "ftn_context_rows_form", "ftn_context_through_weight", "ftn_embed_add",
               "ftn_embed_add_form")


def test_exports_and_abi_version(ftn):
    lib = ftn.lib.load()
    assert lib.ftn_abi_version() == 14 and ftn.lib.ABI_VERSION == 14
    assert set(ENTRY_NAMES) <= set(ftn.lib.EXPORTS)
    for name in ENTRY_NAMES:
        assert hasattr(lib, name)


def test_parameter_blocks_mirror_the_header(ftn):
    """16 pointers, 3 floats, 7 ints / 9 pointers, a float, an int: the sizes the C structs have on a 64-bit ABI."""
    assert C.sizeof(ftn.lib.FtnContextParams) == 16 * 8 + 3 * 4 + 7 * 4
    assert C.sizeof(ftn.lib.FtnEmbedAddParams) == 9 * 8 + 4 + 4
    header = (ROOT / "include" / "flowtimes.h").read_text()
    for struct in (ftn.lib.FtnContextParams, ftn.lib.FtnEmbedAddParams):
        assert f"}} {struct.__name__};" in header


# ------------------------------------------------------------------------------------------------------------ forms
def rows_rule(F, Ws, Ed, R, steps):
    """``ftn_context_rows_form`` restated: element ``lane + 64 j`` of a row vector is slot j of a lane, so a context
    vector takes ceil(ctx / 64) slots, the static projection ceil(Ws / 64), and the late head walks its steps 64 at
    a time."""
    return -(-(Ws + Ed) // 64), -(-Ws // 64), min(-(-steps // 64), 255)


def add_rule(D, qc_bs, qb_bs, mis):
    """``embed_add_form`` restated: a lane holds 4 columns per 256 of d_model; 16-byte loads need whole quads."""
    vec = qc_bs % 4 == 0 and qb_bs % 4 == 0 and mis == 0
    return f"k_embed_add<{1 if D <= 256 else 2},{'true' if vec else 'false'}>"


def test_rows_forms_over_the_table(ftn):
    rt, seen = ftn.runtime, set()
    for F, (Ws, Ed), R, steps in itertools.product((1, 7, 64, 256), ((5, 6), (0, 32), (16, 0), (64, 32), (128, 128),
                                                                       (65, 0), (256, 0)), (0, 1, 32), (0, 1, 64, 65, 96, 20000)):
        got = rt.context_rows_form_of(F, Ws, Ed, R, steps)
        assert got == rows_rule(F, Ws, Ed, R, steps), (F, Ws, Ed, R, steps)
        seen.add(got)
    assert {s[0] for s in seen} == {1, 2, 4} and {s[2] for s in seen} == {0, 1, 2, 255}
    assert ftn.lib.load().ftn_context_rows_form(8, 16, 32, 8, 96) == 1 | 1 << 4 | 2 << 8


def test_embed_add_forms_over_the_table(ftn):
    rt, seen = ftn.runtime, set()
    for D, qc, qb, mis in itertools.product((4, 16, 132, 256, 260, 512), (0, 8 * 256, 3 * 5), (0, 64, 7), (0, 4, 8, 12)):
        got = rt.embed_add_form_of(D, qc, qb, mis)
        assert got == add_rule(D, qc, qb, mis), (D, qc, qb, mis)
        seen.add(got)
    assert seen == {f"k_embed_add<{no},{vec}>" for no in (1, 2) for vec in ("true", "false")}
    lib = ftn.lib.load()
    assert lib.ftn_embed_add_form(256, 0, 0, 0) == 2 | 1 << 4 and lib.ftn_embed_add_form(260, 0, 0, 4) == 2 << 4


def test_form_queries_reject_bad_arguments(ftn):
    rt = ftn.runtime
    for args in [(1, 0, 0, 0, 0), (1, 200, 57, 0, 0), (0, 5, 6, 0, 0), (257, 5, 6, 0, 0), (1, 5, 6, 33, 0),
                 (1, 5, 6, 1, -1), (1, 257, 0, 0, 0)]:
        with pytest.raises(ValueError, match="ftn_context_rows_form"):
            rt.context_rows_form_of(*args)
    for args in [(0, 0, 0, 0), (130, 0, 0, 0), (516, 0, 0, 0), (64, 0, 0, 3), (64, 0, 0, 16)]:
        with pytest.raises(ValueError, match="ftn_embed_add_form"):
            rt.embed_add_form_of(*args)


# ---------------------------------------------------------------------------------------- argument checks of the entries
A, M, H = 0x10000, 0x10004, 0x10002        # stand-ins for device addresses: aligned / 4 bytes on / 2 bytes on
ROW_PTRS = ("w_s", "b_s", "sn_g", "sn_b", "emb", "cn_g", "cn_b", "w_c", "b_c", "w_p", "b_p", "ln_g", "ln_b", "w_l",
            "b_l", "gate")
ADD_PTRS = ("pos", "w_t", "b_t", "aux_g", "aux_b", "gate", "b_v", "basisc", "scale")


def _rows(lib, ftn, a):
    p = ftn.lib.FtnContextParams()
    for name in ROW_PTRS:
        setattr(p, name, a.get(name, A))
    for name in ("F", "Ws", "Ed", "V", "R", "steps"):
        setattr(p, name, a[name])
    p.sn_eps = p.cn_eps = p.ln_eps = 1e-5
    return lib.ftn_context_rows(C.byref(p) if a.get("params", True) else None, a["static"], 0, a["ids"], 0, a["Bc"],
                                a["N"], a["rows"], a["coeff"], a["cbias"], a["late"], None)


def _through(lib, ftn, a):
    return lib.ftn_context_through_weight(a["coeff"], a["cbias"], a["Bc"], a["N"], a["R"], a["w"], a["ldw"], a["D"],
                                          a["qc"], a["qb"], None)


def _add(lib, ftn, a):
    p = ftn.lib.FtnEmbedAddParams()
    for name in ADD_PTRS:
        setattr(p, name, a.get(name, A))
    p.T, p.aux_eps = a["T"], 1e-5
    return lib.ftn_embed_add(C.byref(p) if a.get("params", True) else None, a["mark"], a["mark_bs"], a["qc"], 0, a["R"],
                             a["qb"], 0, a["Ba"], a["L"], a["D"], a["out"], None)


ENTRIES = {
    "ftn_context_rows": (_rows, dict(F=8, Ws=16, Ed=32, V=10, R=8, steps=7, static=A, ids=A, Bc=2, N=5, rows=A, coeff=A,
                                     cbias=A, late=A), {
        "null params": dict(params=False), "null static": dict(static=None), "null ids": dict(ids=None),
        "null W_s": dict(w_s=None), "null table": dict(emb=None), "null context_norm": dict(cn_g=None),
        "null W_c": dict(w_c=None), "null w_p": dict(w_p=None), "null late norm": dict(ln_b=None),
        "null gate": dict(gate=None), "no output": dict(rows=None, coeff=None, cbias=None, late=None),
        "gamma without beta": dict(sn_b=None), "R = 33": dict(R=33), "R = 0": dict(R=0),
        "ctx = 257": dict(Ws=129, Ed=128), "Ws = 257": dict(Ws=257, Ed=0), "F = 257": dict(F=257), "F = 0": dict(F=0),
        "steps = 0": dict(steps=0), "V = 0": dict(V=0), "Bc = 0": dict(Bc=0), "N = 0": dict(N=0),
        "no context": dict(Ws=0, Ed=0), "rows misaligned": dict(rows=H), "coeff misaligned": dict(coeff=H),
        "ids misaligned": dict(ids=M), "static misaligned": dict(static=H)}),
    "ftn_context_through_weight": (_through, dict(coeff=A, cbias=A, Bc=2, N=5, R=8, w=A, ldw=5, D=64, qc=A, qb=A), {
        "null w": dict(w=None), "null coeff": dict(coeff=None), "null cbias": dict(cbias=None),
        "no output": dict(qc=None, qb=None), "R = 33": dict(R=33), "R = 0": dict(R=0), "D = 130": dict(D=130),
        "D = 516": dict(D=516), "D = 0": dict(D=0), "N = 0": dict(N=0), "Bc = 0": dict(Bc=0),
        "row stride < N": dict(ldw=4), "Bc over the grid": dict(Bc=65536, N=65, ldw=65),
        "q_coeff misaligned": dict(qc=H), "q_bias misaligned": dict(qb=H), "w misaligned": dict(w=H)}),
    "ftn_embed_add": (_add, dict(T=4, mark=A, mark_bs=0, qc=A, R=8, qb=A, Ba=2, L=24, D=64, out=A), {
        "null params": dict(params=False), "null out": dict(out=None), "null value bias": dict(b_v=None),
        "null W_t": dict(w_t=None), "null basis": dict(basisc=None), "null scale": dict(scale=None),
        "no term": dict(pos=None, mark=None, aux_g=None, aux_b=None, gate=None, qc=None, qb=None),
        "mark without pos": dict(pos=None, aux_g=None, aux_b=None, gate=None),
        "gamma without gate": dict(gate=None), "R = 33": dict(R=33), "R = 0": dict(R=0), "D = 130": dict(D=130),
        "D = 516": dict(D=516), "D = 0": dict(D=0), "time_dim = 65": dict(T=65), "time_dim = 0": dict(T=0),
        "L = 0": dict(L=0), "Ba = 0": dict(Ba=0), "out misaligned": dict(out=M), "out off by 8": dict(out=A + 8),
        "pos misaligned": dict(pos=H), "mark stride": dict(mark_bs=-4)}),
}
CASES = [(entry, name) for entry, (_, _, bad) in ENTRIES.items() for name in bad]


@pytest.mark.parametrize("entry,name", CASES, ids=[f"{e[4:]}-{n}" for e, n in CASES])
def test_entries_reject_bad_arguments_before_any_launch(entry, name, ftn):
    """None of these reaches a launch (this test runs without a device): non-zero return, and the last error starts
    with the entry's name."""
    lib = ftn.lib.load()
    call, good, bad = ENTRIES[entry]
    assert lib.ftn_embed_add_form(64, 0, 0, 0) > 0                       # leaves an earlier message out of the way
    rc = call(lib, ftn, {**good, **bad[name]})
    assert rc < 0
    msg = lib.ftn_last_error().decode()
    assert msg.startswith(entry + ":"), msg
    with pytest.raises(ValueError, match=entry):
        ftn.lib.check(rc, entry)


# ------------------------------------------------------------------------------------------------------- the switch
_PROBE = textwrap.dedent("""
    import sys
    sys.path.insert(0, {root!r})
    import torch
    import __graft_entry__ as ge
    ftn = ge.load_package()

    class DeviceWindow:                    # what the predicates read of a contiguous fp32 [2, 8, 3] window on a device
        is_cuda, dtype, requires_grad, device = True, torch.float32, False, "cuda:0"
        def stride(self, i): return (24, 3, 1)[i]
        def size(self, i): return (2, 8, 3)[i]

    net = ftn.models.TimesNet(input_len=8, pred_len=2, d_model=16, n_layers=1, k_periods=1, kernel_set=[(3, 3)],
                              dropout=0.0, activation="gelu", mode="direct", id_embed_dim=6, static_proj_dim=5,
                              use_zero_mean_context=True, context_rank=4, use_constant_context_bias=True).eval()
    static, ids = torch.rand(3, 7), torch.tensor([2, 0, 1])
    with torch.inference_mode():
        net(torch.rand(2, 8, 3) + 1.0, series_static=static, series_ids=ids)
        assert net._last_context_backend == "torch"                      # CPU tensors: the torch composition
        w = DeviceWindow()
        print("CTX_OK", int(net._hip_rows_ok(w, static)), int(net._hip_epilogue_ok(w, None)),
              int(net._hip_rows_ok(w, static.double())), int(ftn.models.shell._CTX_HIP))
""")


@pytest.mark.parametrize("value,want", [(None, "CTX_OK 1 1 0 1"), ("1", "CTX_OK 1 1 0 1"), ("0", "CTX_OK 0 0 0 0")])
def test_ctx_switch_restores_the_torch_front_end(value, want):
    """``FTN_CTX_HIP=0`` (read once per process): the rows and the embedding's ``add`` compose torch ops again."""
    env = {k: v for k, v in os.environ.items() if k != "FTN_CTX_HIP"}
    if value is not None:
        env["FTN_CTX_HIP"] = value
    r = subprocess.run([sys.executable, "-c", _PROBE.format(root=str(ROOT))], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip().splitlines()[-1] == want
