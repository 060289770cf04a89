"""The form rule of ``ftn_refit_update`` pinned over the shape table of tests/refit_oracle.py and on both sides of the
threshold between ``k_refit_one`` and the grid, a misaligned operand pinned to the scalar form of its tensor, the
workspace formula, the chunk cap, and the argument errors of the form query and of the launch entry before any launch
(no GPU: host-only queries and stand-in addresses)."""
import ctypes as C
import re

import pytest

import refit_oracle as oracle
from conftest import ROOT

ONE, GRID = "k_refit_one", "k_refit_norm+k_refit_apply"


def test_form_table_over_the_shape_table(ftn):
    """Units of 4 elements per tensor, chunks of 1024 units, one workgroup up to 2 chunks."""
    rt, lib = ftn.runtime, ftn.lib.load()
    want = {(1,): (ONE, 1), (4097,): (ONE, 2), (1023, 4097): (ONE, 2), (4097, 4097): (GRID, 3),
            (193, 255, 256, 257, 1023, 4097): (ONE, 2), (4097, 4097, 4097, 4097, 1, 3): (GRID, 5),
            (4097, 1023, 7, 4097, 5, 4097): (GRID, 4), (4097, 4097, 4097, 4097, 4097, 7, 193, 1023): (GRID, 6),
            (4097, 1, 4097, 3, 4097, 5, 4097, 4097): (GRID, 6)}
    seen = set()
    for counts in oracle.TABLE:
        name, mask, chunks = rt.refit_update_form_of(counts)
        assert (name, mask, chunks) == (oracle.form_name(counts), 0, oracle.chunks(counts)), counts
        if counts in want:
            assert (name, chunks) == want[counts], counts
        arr = (C.c_longlong * len(counts))(*counts)
        assert lib.ftn_refit_update_workspace(len(counts), arr) == 8 * chunks + 16
        seen.add(name)
    assert seen == {ONE, GRID} and set(want) <= set(oracle.TABLE)
    assert {len(c) for c in oracle.TABLE} == {1, 2, 6, 8}
    assert {n for c in oracle.TABLE for n in c} == {1, 3, 4, 5, 7, 64, 193, 255, 256, 257, 1023, 4097}


def test_both_sides_of_the_threshold(ftn):
    """2 chunks = 2048 units = 8192 elements of one tensor are the last total of ``k_refit_one``."""
    rt = ftn.runtime
    assert rt.refit_update_form_of([330]) == (ONE, 0, 1)
    assert rt.refit_update_form_of([64, 1, 64, 1, 7 * 28, 7]) == (ONE, 0, 1)   # the pipeline layout's six tensors
    assert rt.refit_update_form_of([8192]) == (ONE, 0, 2)
    assert rt.refit_update_form_of([8193]) == (GRID, 0, 3)
    assert rt.refit_update_form_of([8189, 1]) == (GRID, 0, 3)              # a tail unit counts as a unit
    assert rt.refit_update_form_of([4096, 4096]) == (ONE, 0, 2)
    assert rt.refit_update_form_of([16384]) == (GRID, 0, 4)
    assert rt.refit_update_form_of([96 * 336, 96, 64, 1, 64, 1]) == (GRID, 0, 8)


def test_a_misaligned_operand_pins_its_tensor_to_the_scalar_form(ftn):
    rt, lib = ftn.runtime, ftn.lib.load()
    assert rt.refit_update_form_of([64, 257, 5], [0, 4, 0]) == (ONE, 0b010, 1)
    assert rt.refit_update_form_of([64, 257, 5], [8, 0, 12]) == (ONE, 0b101, 1)
    assert rt.refit_update_form_of([20000, 7], [4, 0]) == (GRID, 0b01, 5)   # the chunks do not depend on it
    assert rt.refit_update_form_of([20000, 7], None) == (GRID, 0, 5)
    arr = (C.c_longlong * 2)(20000, 7)
    assert lib.ftn_refit_update_form(2, arr, (C.c_int * 2)(4, 0)) == ftn.lib.FTN_REFIT_GRID | 1 << 4 | 5 << 12
    with pytest.raises(ValueError, match="misalign"):
        rt.refit_update_form_of([64], [2])                                  # off the 4-byte grid: no form
    with pytest.raises(ValueError, match="misalign values for 1 tensors"):
        rt.refit_update_form_of([64], [0, 0])


def test_chunks_are_capped(ftn):
    rt = ftn.runtime
    assert ftn.lib.FTN_REFIT_PARTS_MAX == 1024
    assert rt.refit_update_form_of([4096 * 1024])[2] == 1024
    assert rt.refit_update_form_of([4096 * 1024 + 1])[2] == 820            # chunks of 1280 units
    assert rt.refit_update_form_of([2 ** 31 - 1])[2] == 1024
    with pytest.raises(ValueError, match="units of 4"):
        rt.refit_update_form_of([2 ** 31 - 1] * 8)


def test_every_kernel_of_the_file_is_named(ftn):
    text = (ROOT / "flow-timesnet_amd" / "csrc" / "refit.hip").read_text()
    kernels = set(re.findall(r"__global__[^\n]*\bvoid (k_\w+)\(", text))
    assert kernels == {"k_refit_one", "k_refit_norm", "k_refit_apply"}


def test_bad_counts_are_refused_before_any_launch(ftn):
    """More than 8 tensors and an empty tensor: by the form query, by the workspace query (0) and by the launch entry,
    whose check comes before anything is enqueued (the addresses here are stand-ins nothing may touch)."""
    rt, lib, L = ftn.runtime, ftn.lib.load(), ftn.lib
    with pytest.raises(ValueError, match=r"n=9 tensors \(1\.\.8\)"):
        rt.refit_update_form_of([4] * 9)
    with pytest.raises(ValueError, match="every count >= 1"):
        rt.refit_update_form_of([4, 0, 4])
    with pytest.raises(ValueError, match="every count >= 1"):
        rt.refit_update_form_of([-3])
    with pytest.raises(ValueError, match=r"n=0 tensors"):
        rt.refit_update_form_of([])
    assert lib.ftn_refit_update_workspace(9, (C.c_longlong * 9)(*[4] * 9)) == 0
    assert lib.ftn_refit_update_workspace(2, (C.c_longlong * 2)(4, 0)) == 0

    def args(n=2, counts=(8, 8)):
        a = L.FtnRefitArgs()
        for i in range(min(n, 8)):
            a.p[i], a.g[i], a.m[i], a.v[i] = (0x10000 * (4 * i + k + 1) for k in range(4))
            a.n[i] = counts[i] if i < len(counts) else 8
        a.n_tensors = n
        a.beta1, a.beta2, a.eps = 0.9, 0.999, 1e-8
        a.lr, a.state = 0x900000, 0x900100
        return a

    def refused(a, match):
        with pytest.raises(ValueError, match=match):
            L.check(lib.ftn_refit_update(C.byref(a), None), "ftn_refit_update")

    refused(args(n=9), r"9 tensors \(1\.\.8\)")
    refused(args(n=0), r"0 tensors \(1\.\.8\)")
    refused(args(counts=(8, 0)), r"tensor 1 has 0 elements")
    a = args()
    a.g[1] = None
    refused(a, "tensor 1 has a null operand")
    a = args()
    a.m[0] = 0x10002
    refused(a, "off the 4-byte grid")
    a = args()
    a.beta2 = 1.0
    refused(a, "beta2=1")
    a = args()
    a.n_skip = 1
    refused(a, "skip word 0 is null")
    a = args()
    a.n_skip = 9
    refused(a, r"9 skip words \(0\.\.8\)")
    a = args()
    a.log_cap = 4
    refused(a, "log of 4 rows with no buffer")
    a = args()
    a.state = None
    refused(a, "lr word and state")
    a = args(counts=(20000, 8))                                            # the grid form needs its workspace
    refused(a, "workspace of 0 bytes, 56 needed")
    a = args(counts=(70000 * 4, 8))
    a.force_form = L.FTN_REFIT_ONE
    refused(a, "force_form=1 with 69 chunks")
    a = args()
    a.force_form = 3
    refused(a, "force_form=3")
