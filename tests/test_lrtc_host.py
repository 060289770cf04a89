"""The low-rank temporal context's host side (``ftn_lrtc_form``, the argument checks of ``ftn_lrtc_forward``, the
shape handling of ``LowRankTemporalContext.forward`` on the torch branch): no GPU needed.  The form rule is restated
here and compared over a table; every argument error must be reported, with a message, before anything touches a
device."""
import itertools

import pytest
import torch

RS = (1, 3, 4, 5, 8, 9, 16, 17, 31, 32)
NS = (1, 3, 4, 5, 64, 252, 256, 257, 260, 512, 513, 768, 769, 1024, 1028, 2052, 4096)
# (out | x) & 15 in the low nibble, coeff & 15 in the high one
MIS = (0x00, 0x04, 0x08, 0x0c, 0x40, 0x80, 0xc0, 0x44, 0xc8)


def form_rule(N, R, addx, mis):
    """``lrtc_form`` (csrc/lrtc.hip) restated: the rank padded to 4 / 8 / 16 / 32; vector stores when the rows are
    whole quads and out (and x) aligned; wide coefficient loads when the rank fills its padding, a whole quad exists
    and coeff is aligned; 64-lane groups enough for ceil(N / 4) quads, 192 rounded up, 256 at the most."""
    rt = 4 if R <= 4 else 8 if R <= 8 else 16 if R <= 16 else 32
    vec = N % 4 == 0 and mis & 15 == 0
    wide = R == rt and N >= 4 and mis & 0xf0 == 0
    quads = -(-N // 4)
    nqb = min(256, -(-quads // 64) * 64)
    nqb = 256 if nqb == 192 else nqb
    tf = ("false", "true")
    return f"k_lrtc<{rt},{tf[vec]},{tf[bool(addx)]}>", wide, nqb


def test_form_rule_over_the_table(ftn):
    rt = ftn.runtime
    seen = set()
    for N, R, addx, mis in itertools.product(NS, RS, (False, True), MIS):
        got = rt.lrtc_form_of(N, R, addx, mis)
        assert got == form_rule(N, R, addx, mis), (N, R, addx, mis, got)
        seen.add(got)
    tf = ("false", "true")
    assert {s[0] for s in seen} == {f"k_lrtc<{r},{v},{a}>" for r in (4, 8, 16, 32) for v in tf for a in tf}
    assert {s[1] for s in seen} == {False, True} and {s[2] for s in seen} == {64, 128, 256}


def test_form_encoding(ftn):
    """The raw value: bit 0 vector stores, bit 1 the fused add, bit 2 wide coefficient loads, RT in bits 4-9, nqb / 64
    in bits 12-15."""
    lib = ftn.lib.load()
    assert lib.ftn_lrtc_form(4096, 16, 1, 0) == 1 | 2 | 4 | 16 << 4 | 4 << 12
    assert lib.ftn_lrtc_form(4096, 16, 0, 0x40) == 1 | 16 << 4 | 4 << 12          # coeff off a boundary: not wide
    assert lib.ftn_lrtc_form(4096, 16, 1, 0x04) == 2 | 4 | 16 << 4 | 4 << 12      # out or x off a boundary: not vec
    assert lib.ftn_lrtc_form(5, 4, 0, 0) == 4 | 4 << 4 | 1 << 12                  # one whole quad, then a tail
    assert lib.ftn_lrtc_form(3, 1, 0, 0) == 4 << 4 | 1 << 12
    assert lib.ftn_lrtc_form(768, 32, 0, 0) == 1 | 4 | 32 << 4 | 4 << 12          # 192 lanes round up to 256
    assert lib.ftn_lrtc_form(260, 9, 1, 0) == 1 | 2 | 16 << 4 | 2 << 12


@pytest.mark.parametrize("args", [(0, 4, 0, 0), (4, 0, 0, 0), (4, 33, 0, 0), (4, 4, 2, 0), (4, 4, -1, 0),
                                  (4, 4, 0, 2), (4, 4, 0, 0x20), (4, 4, 0, 256), (4, 4, 0, -4)])
def test_form_rejects_bad_arguments(args, ftn):
    lib = ftn.lib.load()
    assert lib.ftn_lrtc_form(*args) < 0
    assert b"ftn_lrtc_form" in lib.ftn_last_error()
    with pytest.raises(ValueError, match="ftn_lrtc_form"):
        ftn.runtime.lrtc_form_of(*args)


A, M = 0x10000, 0x10004          # stand-ins for device addresses: 16-byte aligned / 4 bytes past a boundary
GOOD = dict(coeff=A, basis=A, scale=A, x=None, out=A, B=2, L=24, N=5, R=4)
BAD = {
    "null coeff": dict(coeff=None), "null basis": dict(basis=None), "null scale": dict(scale=None),
    "null out": dict(out=None), "B = 0": dict(B=0), "L = 0": dict(L=0), "N = 0": dict(N=0), "R = 0": dict(R=0),
    "N < 0": dict(N=-4), "R = 33": dict(R=33), "B beyond gridDim.z": dict(B=65536),
    "L beyond gridDim.y": dict(L=48 * 65535 + 1), "coeff off a float": dict(coeff=A + 2), "x off a float": dict(x=A + 1),
    "out off a float": dict(out=M + 2),
}


@pytest.mark.parametrize("name", list(BAD))
def test_forward_rejects_bad_arguments_before_any_launch(name, ftn):
    """None of these reaches a launch (this test runs without a device): non-zero return, and the last error names
    the entry point."""
    lib = ftn.lib.load()
    a = {**GOOD, **BAD[name]}
    assert lib.ftn_lrtc_form(5, 4, 0, 0) > 0                            # leaves an earlier message out of the way
    rc = lib.ftn_lrtc_forward(a["coeff"], a["basis"], a["scale"], a["x"], a["out"], a["B"], a["L"], a["N"], a["R"], None)
    assert rc != 0
    msg = lib.ftn_last_error().decode()
    assert msg.startswith("ftn_lrtc_forward"), msg
    with pytest.raises(ValueError, match="ftn_lrtc_forward"):
        ftn.lib.check(rc, "ftn_lrtc_forward")


def test_exports_keep_the_abi_number(ftn):
    lib = ftn.lib.load()
    assert lib.ftn_abi_version() == 14 and ftn.lib.ABI_VERSION == 14
    assert {"ftn_lrtc_forward", "ftn_lrtc_form", "ftn_lrtc_basis"} <= set(ftn.lib.EXPORTS)


def test_wrapper_validates_layout_on_the_host(ftn):
    rt = ftn.runtime
    with pytest.raises(ValueError, match="coeff"):
        rt.lrtc_forward(torch.zeros(2, 5, 4), 24, torch.ones(1), None)          # not on a device
    with pytest.raises(ValueError, match="coeff"):
        rt.lrtc_forward(torch.zeros(5, 4), 24, torch.ones(1), None)


ADD_SHAPES = {"none": None, "dense": (2, 6, 5), "[1, L, N]": (1, 6, 5), "[L, N]": (6, 5), "[B, 1, 1]": (2, 1, 1),
              "[N]": (5,), "scalar": (), "[3, B, L, N]": (3, 2, 6, 5)}


@pytest.mark.parametrize("name", list(ADD_SHAPES))
def test_torch_branch_adds_as_torch_adds(name, ftn):
    """What the HIP branch must reproduce (tests/test_gpu_lrtc.py): on the CPU ``forward`` is ``add_to + ctx``."""
    mod = ftn.models.LowRankTemporalContext(4, 0.5).eval()
    g = torch.Generator().manual_seed(7)
    coeff = torch.randn(2, 5, 4, generator=g)
    shape = ADD_SHAPES[name]
    add = None if shape is None else torch.randn(shape, generator=g)
    with torch.no_grad():
        ctx = mod(coeff, 6)
        got = mod(coeff, 6, add_to=add)
    assert mod._last_backend == "torch"
    assert torch.equal(got, ctx if add is None else add + ctx)


@pytest.mark.parametrize("shape", [(2, 6, 4), (2, 5, 5), (3, 6, 5), (2, 6, 5, 1)])
def test_torch_branch_rejects_what_torch_rejects(shape, ftn):
    mod = ftn.models.LowRankTemporalContext(4, 0.5).eval()
    coeff = torch.zeros(2, 5, 4)
    with torch.no_grad(), pytest.raises(RuntimeError, match="must match the size"):
        mod(coeff, 6, add_to=torch.zeros(shape))
