"""The form rule of ``ftn_timeproj_backward`` pinned over the shape grid of tests/test_gpu_output_fit.py, its workspace
formula, the chunk cap, and the argument errors of the form query, the workspace query and the launch entry before any
launch (no GPU: host-only queries and stand-in addresses)."""
import re

import pytest
import torch

import output_fit_oracle as oracle
from conftest import ROOT


def test_the_grid_covers_every_axis_value_within_the_size_limit():
    assert len(oracle.GRID) == 36 and all(B * L * D <= 2 ** 20 for B, L, _, D in oracle.GRID)
    for k, axis in enumerate((oracle.BS, oracle.LS, oracle.SS, oracle.DS)):
        assert {c[k] for c in oracle.GRID} == set(axis)


def test_form_table_over_the_grid(ftn):
    """One form; chunks of 8 batch rows; a partial of [S][L + 1] floats per chunk."""
    rt, lib = ftn.runtime, ftn.lib.load()
    assert ftn.lib.TIMEPROJ_BWD_CHUNK == oracle.C == 8
    want = {1: 1, 2: 1, 3: 1, 7: 1, 8: 1, 9: 2, 19: 3}
    for B, L, S, D in oracle.GRID:
        assert rt.timeproj_backward_form_of(B, L, S, D) == ("k_timeproj_bwd_mfma", want[B]), (B, L, S, D)
        assert lib.ftn_timeproj_backward_form(B, L, S, D, 0) == ftn.lib.FTN_TIMEPROJ_BWD_MFMA | want[B] << 4
        assert lib.ftn_timeproj_backward_workspace(B, L, S, D) == want[B] * S * (L + 1) * 4
    # the shapes DESIGN times: the pipeline layout, the bench shape, a configs[4] shard
    assert rt.timeproj_backward_form_of(4096, 28, 7, 64) == ("k_timeproj_bwd_mfma", 256)
    assert rt.timeproj_backward_form_of(256, 336, 96, 64) == ("k_timeproj_bwd_mfma", 32)
    assert rt.timeproj_backward_form_of(64, 720, 96, 128) == ("k_timeproj_bwd_mfma", 8)


def test_every_form_the_kernel_file_defines_is_named(ftn):
    text = (ROOT / "flow-timesnet_amd" / "csrc" / "timeproj_bwd.hip").read_text()
    kernels = set(re.findall(r"__global__[^\n]*\bvoid (k_\w+)\(", text))
    assert kernels - {"k_timeproj_bwd_reduce"} == oracle.FORMS


def test_chunks_are_capped(ftn):
    """Beyond 256 chunks of 8 batch rows the chunk grows."""
    rt, lib = ftn.runtime, ftn.lib.load()
    assert ftn.lib.FTN_TIMEPROJ_BWD_CHUNKS_MAX == 256
    assert rt.timeproj_backward_form_of(2048, 28, 7, 64)[1] == 256
    assert rt.timeproj_backward_form_of(2049, 28, 7, 64)[1] == 228          # chunks of 9 rows
    assert rt.timeproj_backward_form_of(4097, 28, 7, 64)[1] == 241          # chunks of 17 rows
    assert rt.timeproj_backward_form_of(1 << 30, 1, 1, 4)[1] == 256
    assert lib.ftn_timeproj_backward_workspace(2049, 28, 7, 64) == 228 * 7 * 29 * 4


@pytest.mark.parametrize("args", [(0, 28, 7, 64, 0), (4, 0, 7, 64, 0), (4, 28, 0, 64, 0), (4, 28, 7, 0, 0),
                                  (4, 28, 7, 66, 0), (4, 28, 7, 516, 0), (4, 28, 7, 64, 3), (4, 28, 7, 64, 16),
                                  (4, 28, 7, 64, 4), (-1, 28, 7, 64, 0), (4, 1 << 30, 1 << 30, 64, 0)])
def test_form_and_workspace_reject_bad_arguments(args, ftn):
    lib = ftn.lib.load()
    assert lib.ftn_timeproj_backward_form(4, 28, 7, 64, 0) > 0
    assert lib.ftn_timeproj_backward_form(*args) < 0
    assert lib.ftn_last_error().decode().startswith("ftn_timeproj_backward_form")
    assert lib.ftn_timeproj_backward_workspace(*args[:4]) == 0 or args[4] != 0
    with pytest.raises(ValueError, match="ftn_timeproj_backward_form"):
        ftn.runtime.timeproj_backward_form_of(*args)


A, M = 0x10000, 0x10004          # stand-ins for device addresses: 16-byte aligned / 4 bytes past a boundary
GOOD = dict(seq=A, dh=A, B=9, L=5, S=3, D=8, dw=A, db=A, wsp=A, wsb=2 * 3 * 6 * 4)
BAD = {
    "null seq": dict(seq=None), "null d_hidden": dict(dh=None), "null dW_t": dict(dw=None), "null db_t": dict(db=None),
    "null workspace": dict(wsp=None), "B = 0": dict(B=0), "L = 0": dict(L=0), "S = 0": dict(S=0), "D = 6": dict(D=6),
    "D = 0": dict(D=0), "D = 516": dict(D=516), "seq off by 4": dict(seq=M), "d_hidden off by 8": dict(dh=A + 8),
    "dW_t off by 2": dict(dw=A + 2), "db_t off by 1": dict(db=A + 1), "workspace off by 2": dict(wsp=A + 2),
    "workspace too small": dict(wsb=2 * 3 * 6 * 4 - 4), "workspace of one chunk": dict(wsb=3 * 6 * 4),
}


@pytest.mark.parametrize("name", list(BAD))
def test_launch_entry_rejects_bad_arguments_before_any_launch(name, ftn):
    lib = ftn.lib.load()
    a = {**GOOD, **BAD[name]}
    assert lib.ftn_timeproj_backward_workspace(9, 5, 3, 8) == GOOD["wsb"]       # (and clears an earlier message's way)
    assert lib.ftn_head_backward_form(8, 2, 8, 0) > 0
    rc = lib.ftn_timeproj_backward(a["seq"], a["dh"], a["B"], a["L"], a["S"], a["D"], a["dw"], a["db"], a["wsp"],
                                   a["wsb"], None)
    assert rc < 0 and lib.ftn_last_error().decode().startswith("ftn_timeproj_backward:")
    with pytest.raises(ValueError, match="ftn_timeproj_backward"):
        ftn.lib.check(rc, "ftn_timeproj_backward")


def test_wrapper_validates_on_the_host_and_the_abi_stays(ftn):
    rt = ftn.runtime
    z = torch.zeros
    with pytest.raises(ValueError, match="seq must be a contiguous fp32 device tensor"):
        rt.timeproj_backward(z(2, 5, 8), z(2, 3, 8))
    with pytest.raises(ValueError, match=r"takes seq \[B, L, D\] and d_hidden \[B, S, D\]"):
        rt.timeproj_backward(z(2, 5, 8), z(3, 3, 8))
    assert {"ftn_timeproj_backward", "ftn_timeproj_backward_form", "ftn_timeproj_backward_workspace"} <= set(ftn.lib.EXPORTS)
    assert ftn.lib.ABI_VERSION == 14 and ftn.lib.load().ftn_abi_version() == 14
