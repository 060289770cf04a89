"""The host side of the RMS norm epilogue of the value embedding (``ftn_embed_forward_rms``, ``ftn_embed_ring_rms`` and
their wide counterparts; csrc/shell_api.hip): exports, every argument error reported with the entry's
name before anything touches a device, the fourth element of ``runtime``'s ``norm`` tuple, and the torch path a CPU
model keeps.  No GPU needed."""
import pytest
import torch

from test_dropin_reference import SHELL_CASES, _fixture, _part

RMS = ("ftn_embed_forward_rms", "ftn_embed_ring_rms", "ftn_embed_wide_forward_rms", "ftn_embed_wide_ring_rms")
A, M = 0x10000, 0x10004          # stand-ins for device addresses: 16-byte aligned / 4 bytes past a boundary


def test_exports_and_abi_version(ftn):
    lib = ftn.lib.load()
    assert lib.ftn_abi_version() == 14 and ftn.lib.ABI_VERSION == 14
    assert set(RMS) <= set(ftn.lib.EXPORTS)
    for name in RMS:
        assert hasattr(lib, name)


def _forward(entry):
    return lambda lib, a: getattr(lib, entry)(a["x"], a["x_bs"], a["B"], a["L"], a["N"], a["w"], a["D"], a["add"],
                                              a["add_bs"], a["g"], a["b"], 1e-5, a["out"], None)


def _ring(entry):
    return lambda lib, a: getattr(lib, entry)(a["V"], a["B"], a["L"], a["D"], a["head"], a["add"], a["add_bs"], a["g"],
                                              a["b"], 1e-5, a["out"], None)


_FWD = dict(x=A, x_bs=24 * 8, B=2, L=24, N=8, w=A, add=A, add_bs=0, g=A, b=A, out=A)
_RNG = dict(V=A, B=2, L=24, head=3, add=A, add_bs=0, g=A, b=A, out=A)
_COMMON = {"null gamma": dict(g=None), "null beta": dict(b=None), "null gamma and beta": dict(g=None, b=None),
           "D % 4": dict(D=30), "D = 0": dict(D=0), "out misaligned": dict(out=M), "gamma misaligned": dict(g=M),
           "null out": dict(out=None), "L = 0": dict(L=0)}
_NARROW_D = {"D = 132": dict(D=132)}
_WIDE_D = {"D = 128": dict(D=128), "D = 516": dict(D=516), "D % 4 wide": dict(D=258)}
ENTRIES = {
    "ftn_embed_forward_rms": (_forward("ftn_embed_forward_rms"), dict(_FWD, D=64),
                              {**_COMMON, **_NARROW_D, "null x": dict(x=None), "add stride": dict(add_bs=6)}),
    "ftn_embed_ring_rms": (_ring("ftn_embed_ring_rms"), dict(_RNG, D=64),
                           {**_COMMON, **_NARROW_D, "head = L": dict(head=24), "V misaligned": dict(V=M)}),
    "ftn_embed_wide_forward_rms": (_forward("ftn_embed_wide_forward_rms"), dict(_FWD, D=256),
                                   {**_COMMON, **_WIDE_D, "null W": dict(w=None), "add misaligned": dict(add=M)}),
    "ftn_embed_wide_ring_rms": (_ring("ftn_embed_wide_ring_rms"), dict(_RNG, D=256),
                                {**_COMMON, **_WIDE_D, "head < 0": dict(head=-1), "null V": dict(V=None)}),
}
CASES = [(entry, name) for entry, (_, _, bad) in ENTRIES.items() for name in bad]


@pytest.mark.parametrize("entry,name", CASES, ids=[f"{e[4:]}-{n}" for e, n in CASES])
def test_entries_reject_bad_arguments_before_any_launch(entry, name, ftn):
    """None of these reaches a launch (this test runs without a device): a negative return, and the last error starts
    with the entry's name."""
    lib = ftn.lib.load()
    call, good, bad = ENTRIES[entry]
    assert lib.ftn_embed_form(8, 64, 0, 0, 0) > 0                         # leaves an earlier message out of the way
    rc = call(lib, {**good, **bad[name]})
    assert rc < 0
    msg = lib.ftn_last_error().decode()
    assert msg.startswith(entry + ":"), msg
    with pytest.raises(ValueError, match=entry):
        ftn.lib.check(rc, entry)


def test_the_layernorm_entries_still_take_no_norm(ftn):
    """Null gamma and beta is "no norm" for the LayerNorm entries and stays so: with them a bad head is what is
    reported, where the RMS entry reports its missing parameters first."""
    lib = ftn.lib.load()
    assert lib.ftn_embed_ring(A, 2, 24, 64, 24, None, 0, None, None, 0.0, A, None) < 0
    assert "head" in lib.ftn_last_error().decode()
    assert lib.ftn_embed_ring_rms(A, 2, 24, 64, 3, None, 0, None, None, 0.0, A, None) < 0
    assert "gamma" in lib.ftn_last_error().decode()


@pytest.mark.parametrize("kind", ["layer", "RMS", "", None, 2])
def test_runtime_rejects_another_fourth_element(kind, ftn):
    """The check comes before the library is asked for anything: CPU tensors do."""
    rt = ftn.runtime
    g, b = torch.ones(8), torch.zeros(8)
    with pytest.raises(ValueError, match="norm"):
        rt.embed_forward(torch.zeros(1, 2, 4), torch.zeros(8, 4), None, (g, b, 1e-5, kind))
    with pytest.raises(ValueError, match="norm"):
        rt.embed_ring(torch.zeros(1, 2, 8), 0, None, (g, b, 1e-5, kind))
    with pytest.raises(ValueError, match="norm"):
        rt.embed_ring(torch.zeros(1, 2, 8), 0, None, (g, b, 1e-5, "rms", "rms"))


def test_a_cpu_rms_model_keeps_the_torch_embedding(ftn):
    cfg, _ = SHELL_CASES["rms_recursive"]
    z = _fixture("rms_recursive")
    x, kw = torch.from_numpy(z["x"]), _part(z, "kw:")
    with torch.no_grad():
        torch.manual_seed(1)
        net = ftn.models.TimesNet(**cfg).eval()
        net(x, **kw)
        net.load_state_dict(_part(z, "sd:"), strict=True)
        net(x, **kw)
    assert net.embedding.embed_norm_mode == "rms" and isinstance(net.embedding.norm, ftn.models.shell.RMSNorm)
    assert net._last_embed_backend == "torch" and net._last_context_backend == "torch"
    assert not net._hip_embed_ok(x) and not net._hip_epilogue_ok(x, None)


def test_the_epilogue_hands_the_rms_parameters_over(ftn):
    """``_embed_epilogue`` names the norm's kind as the fourth element; the series-sharded forward, which has no RMS
    kernel, keeps getting None and applies the module."""
    cfg, _ = SHELL_CASES["rms_recursive"]
    z = _fixture("rms_recursive")
    x, kw = torch.from_numpy(z["x"]), _part(z, "kw:")
    with torch.no_grad():
        net = ftn.models.TimesNet(**cfg).eval()
        net(x, **kw)
        window = x[:, -cfg["input_len"]:]
        _, ln = net._embed_epilogue(window, None)
        assert len(ln) == 4 and ln[3] == "rms" and ln[0] is not None and ln[2] == net.embedding.norm.eps
        assert net.series_embedding_epilogue(window, None)[1] is None
