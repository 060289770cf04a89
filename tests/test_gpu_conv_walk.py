"""The fast conv's row walk (``csrc/ftn_conv_walk.h``) decides which workgroup computes a (tile, batch row), never what
it computes: with the tile switch charged (``FTN_CONV_WALK=1``, the default) and with the equal split (``=0``) the
block must give the same bits.  ``conv_walk_child.py`` runs the cases of its ``CASES`` table in one fresh process per
setting (the library reads the switch once); here the two runs are compared:

* ``y`` and the digest of the whole workspace after the call are equal - the workspace holds a', which stage C
  computed from stage B's output, and stage D's output m', so both conv launches are covered;
* ``y`` matches the fp64 oracle at the tolerance of ``test_gpu_forms.py``;
* the row ranges the stage-D workgroups stamped partition each branch's sequence in both runs, are the equal split
  under ``=0``, and under ``=1`` differ from it where workgroups own several rows (so the switch is not a no-op) while
  no workgroup that walks on into another tile owns more rows than one that does not."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from conv_walk_child import CASES, KS, case_inputs
from test_gpu_forms import ATOL, RTOL, oracle_fp64

pytestmark = pytest.mark.gpu
TESTS = Path(__file__).resolve().parent


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("conv_walk")
    out = {}
    for mode in ("0", "1"):
        path = tmp / f"walk{mode}.npz"
        r = subprocess.run([sys.executable, str(TESTS / "conv_walk_child.py"), str(path)], capture_output=True, text=True,
                           timeout=300, env=dict(os.environ, FTN_CONV_WALK=mode))
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        out[mode] = dict(np.load(path))
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_walks_give_the_same_bits(name, runs):
    a, b = runs["0"], runs["1"]
    want = "k_conv_bf_fast<2,2>" if CASES[name][0] == 128 else "k_conv_bf_fast<2,1>"
    assert str(a[f"conv_{name}"]) == str(b[f"conv_{name}"]) == want
    assert np.array_equal(a[f"y_{name}"], b[f"y_{name}"], equal_nan=True), "y differs between the walks"
    assert str(a[f"ws_{name}"]) == str(b[f"ws_{name}"]), "the workspace (a', m') differs between the walks"


@pytest.mark.parametrize("name", list(CASES))
def test_walk_matches_fp64_oracle(name, runs, ftn):
    C, B, L, periods, seed = CASES[name]
    P, x, amps = case_inputs(ftn, name)
    y_ref, _ = oracle_fp64(x, P, "gelu", 0, L, periods, amps, ks=KS)
    y = runs["1"][f"y_{name}"]
    err = float(np.abs(y - y_ref.numpy()).max())
    print(f"conv_walk {name} B={B} L={L} C={C}: max|y-y64|={err:.3e}")
    np.testing.assert_allclose(y, y_ref.numpy(), rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("name", list(CASES))
def test_stamped_ranges_partition_the_rows(name, runs):
    C, B, L, periods, seed = CASES[name]
    R = 5 * B                                                    # five groups, one tile each
    nvb = 3 * (C // 64)                                          # (branch, output tile) pairs
    for mode in ("0", "1"):
        rows = runs[mode][f"rows_{name}"]
        owners = np.zeros(R, dtype=np.int64)
        for taps, lo, hi in rows:
            assert 0 <= lo < hi <= R
            owners[lo:hi] += 1
        assert (owners == nvb).all(), (mode, owners.tolist())
    eq, sw = runs["0"][f"rows_{name}"], runs["1"][f"rows_{name}"]
    for taps in (9, 25, 49):
        e, s = eq[eq[:, 0] == taps], sw[sw[:, 0] == taps]
        n_most = int((e[:, 2] - e[:, 1]).max())
        assert int((e[:, 2] - e[:, 1]).min()) >= n_most - 1      # the equal split: floor or ceil of R / n
        crossing = s[(s[:, 1] // B) != ((s[:, 2] - 1) // B)]
        inside = s[(s[:, 1] // B) == ((s[:, 2] - 1) // B)]
        if len(crossing) and len(inside):
            assert int((crossing[:, 2] - crossing[:, 1]).max()) <= int((inside[:, 2] - inside[:, 1]).max())
    if name in ("b24", "b52"):
        assert not np.array_equal(eq, sw), "FTN_CONV_WALK changes nothing at this shape"
