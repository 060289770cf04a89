"""Child process of ``test_gpu_conv_walk.py``: the library reads ``FTN_CONV_WALK`` once at load, so each setting runs
here, in a fresh process.  ``python conv_walk_child.py OUT.npz`` runs every case of ``CASES`` through
``ftn_timesblock_forward`` on a zero-filled workspace with a five-group stub selection and writes, per case, ``y``, a
digest of the whole workspace after the call (it holds a' = stage C's output, computed from stage B's, and stage D's
m'), the conv form, and the row range ``[lo, hi)`` every stage-D workgroup stamped (``ftn_debug_stamps``) with its tap
count."""
import ctypes
import hashlib
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

KS = [(3, 3), (5, 5), (7, 7)]
DIVISORS = [4, 6, 12, 16, 24]                    # of L = 48: five grids of 48 pixels, one conv tile each
# name: (d_model, B, L, periods, seed).  At L = 48 a branch's sequence is 5 tiles x B rows on 256 CUs' workgroups:
#   b3    15 rows: most workgroups own none, the others one
#   b24   120 rows: the 3x3 workgroups own several and some walk on into the next tile
#   b52   260 rows: the 7x7 workgroups own two or three, ranges straddle tile boundaries in every branch
#   pad   period 12 of L = 50 leaves 10 pad pixels, period 7 leaves 6
#   wide  d_model 128: k_conv_bf_fast<2,2>, two input groups per row
CASES = {
    "b3": (64, 3, 48, DIVISORS, 61),
    "b24": (64, 24, 48, DIVISORS, 62),
    "b52": (64, 52, 48, DIVISORS, 63),
    "pad": (64, 24, 50, [12, 5, 10, 25, 7], 64),
    "wide": (128, 26, 48, DIVISORS, 65),
}


def case_inputs(ftn, name):
    C, B, L, periods, seed = CASES[name]
    P = {k: torch.from_numpy(v) for k, v in ftn.synth.make_inception_params(C, 4 * C, KS, 4.0, seed=C).items()}
    x = torch.from_numpy(ftn.synth.make_input(B, L, C, seed=seed, planted=()))
    amps = np.random.RandomState(seed).standard_normal(size=(B, len(periods))).astype(np.float32)
    return P, x, amps


def main(out):
    import __graft_entry__ as ge
    from test_gpu_forms import _Stub

    ftn = ge.load_package()
    lib, rt, T = ftn.lib.load(), ftn.runtime, ftn.models.timesnet
    dev = torch.device("cuda:0")
    res = {}
    for name, (C, B, L, periods, seed) in CASES.items():
        P, x, amps = case_inputs(ftn, name)
        blk = T.TimesBlock(C, KS, 0.0, "gelu", d_ff=4 * C, bottleneck_ratio=4.0)
        blk.engine = "f16x2"
        blk.inception.load_state_dict(P, strict=True)
        blk = blk.eval().to(dev)
        object.__setattr__(blk, "period_selector", _Stub(periods, amps))
        wblob, plan = blk._packed(dev)
        xd = x.to(dev)
        sel = blk._select(xd, xd, plan, wblob, None, fuse_a=False)
        assert sel.max_groups == 5
        need = lib.ftn_timesblock_workspace_bytes(ctypes.byref(plan), B, L, sel.max_groups, sel.px_bound)
        st = torch.cuda.current_stream().cuda_stream

        def forward():
            ws = torch.zeros(need, dtype=torch.uint8, device=dev)
            y = torch.full_like(xd, float("nan"))
            flag = torch.zeros(1, dtype=torch.int32, device=dev)
            rc = lib.ftn_timesblock_forward(xd.data_ptr(), y.data_ptr(), B, L, ctypes.byref(plan), wblob.data_ptr(),
                                            sel.desc.data_ptr(), sel.weights.data_ptr(), sel.max_groups, sel.px_bound, 0, 0,
                                            ws.data_ptr(), ws.numel(), st, flag.data_ptr())
            ftn.lib.check(rc, "ftn_timesblock_forward")
            torch.cuda.synchronize()
            assert int(flag.item()) == 0
            return y, ws

        y, ws = forward()
        stamps = torch.zeros(1024 * 8, dtype=torch.int64, device=dev)
        lib.ftn_debug_stamps(stamps.data_ptr(), stamps.numel(), 1)        # both convs stamp; stage D's records stay
        y2, _ = forward()
        lib.ftn_debug_stamps(None, 0, 0)
        assert torch.equal(y2, y)
        s = stamps.cpu().numpy().reshape(-1, 8)
        s = s[s[:, 3] > 0]
        res[f"y_{name}"] = y.cpu().numpy()
        res[f"ws_{name}"] = np.array(hashlib.sha256(ws.cpu().numpy().tobytes()).hexdigest())
        res[f"conv_{name}"] = np.array(rt.timesblock_forms(plan, B, L, 0, 0)["conv"])
        res[f"rows_{name}"] = np.stack([s[:, 4], s[:, 5] >> 32, s[:, 5] & 0xffffffff], 1)
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1])
