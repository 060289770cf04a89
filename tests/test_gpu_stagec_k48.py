"""Layer 1 of the position-major stage C at K = 48 (f16x2, d_model 64, the fragment-prefetch form of stagec_pos.hip):
three 16-channel groups in two K-32 slabs, the second one half padding.  Against the fp64 oracle at the tolerance of
``test_gpu_forms_small.py`` for this engine (rtol 1e-4 / atol 5e-6), at B = 3, L = 40 (three 16-position units per
row, the last one partial; nine units = a partial last workgroup):

* periods that divide L (no tail pixels), periods with pads (tail workgroups: pads 2, 12 and 26 = one and two tail
  units), and seven periods (seven groups: a second pass of the five-group loop);
* ``W_out1`` whole, with only columns 32..47 non-zero and with those columns zero - the bottleneck's third path is
  those columns (pack.py), so slab 1 is then all of layer 1, or none of it: a wrong lane-to-channel map on either
  operand of one slab cannot hide behind the other.  (A form that ran slab 1 as one K-16 MFMA step straight behind
  slab 0's K-32 chain failed exactly the cases with a non-zero slab 0)"""
import functools

import numpy as np
import pytest
import torch

from oracle import timesblock_oracle as orc
from test_gpu_forms import ATOL, KS, RTOL, _Stub, _check, oracle_fp64

C, D_FF, RATIO, ENGINE, ACT = 64, 256, 4.0, "f16x2", "gelu"
B, L = 3, 40
PERIODS = {"nopad": [8, 5, 10], "pads": [7, 13, 33], "seven": [7, 9, 11, 13, 17, 19, 23]}
COLUMNS = ("all", "only_32_47", "zero_32_47")
# W_out1[:, 16 j : 16 j + 16] = proj_j . branch.2 of path j: the columns of a path vanish with its branch.2 weight
ZEROED_PATHS = {"all": (), "only_32_47": (0, 1), "zero_32_47": (2,)}


def _ftn():
    import __graft_entry__ as ge
    return ge.load_package()


@functools.lru_cache(maxsize=None)
def _params(columns):
    sd = _ftn().synth.make_inception_params(C, D_FF, KS, RATIO, seed=48)
    for j in ZEROED_PATHS[columns]:
        sd[f"0.paths.{j}.branch.2.weight"] = np.zeros_like(sd[f"0.paths.{j}.branch.2.weight"])
    return {k: torch.from_numpy(v) for k, v in sd.items()}


def _amps(pset):
    return np.random.RandomState(48).standard_normal(size=(B, len(PERIODS[pset]))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _reference(columns, pset):
    x = torch.from_numpy(_ftn().synth.make_input(B, L, C, seed=48, planted=()))
    y, periods = oracle_fp64(x, _params(columns), ACT, 0, L, PERIODS[pset], _amps(pset))
    return x, y, periods


@pytest.mark.gpu
@pytest.mark.parametrize("pset", list(PERIODS))
@pytest.mark.parametrize("columns", COLUMNS)
def test_k48_layer1_matches_fp64_oracle(columns, pset, ftn):
    dev = torch.device("cuda:0")
    x, y_ref, periods = _reference(columns, pset)
    blk = ftn.models.timesnet.TimesBlock(C, KS, 0.0, ACT, d_ff=D_FF, bottleneck_ratio=RATIO)
    blk.engine = ENGINE
    blk.inception.load_state_dict(_params(columns), strict=True)
    blk = blk.eval().to(dev)
    object.__setattr__(blk, "period_selector", _Stub(periods, _amps(pset)))
    with torch.inference_mode():
        y = blk(x.to(dev))
    assert blk._last_backend == "hip"
    assert blk._last_forms["C"] == "k_mlp_pos64<2>"
    groups = orc.period_group(periods, L, 1, L).periods
    assert blk._last_group_count == len(groups) == len(PERIODS[pset])
    if pset == "seven":
        assert len(groups) > 5                                   # a second pass
    pads = [(-L) % p for p in PERIODS[pset]]
    assert any(pads) == (pset != "nopad")
    err = float((y.double().cpu() - y_ref).abs().max())
    print(f"stagec_k48 {columns} {pset} pads={pads}: max|y-y64|={err:.3e} max|y64|={float(y_ref.abs().max()):.3e}")
    _check(y, y_ref, ENGINE, RTOL, ATOL)
