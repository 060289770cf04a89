"""The form rule of ``ftn_head_backward`` pinned over the R, N, D and misalignment values of tests/test_gpu_fit.py, its
workspace, the argument errors of the two head entries before a launch, and ``table.min_sigma`` on the host side (no GPU): the torch backend against what the reference's own ``_masked_std``
returned (tests/golden/min_sigma_cases.npz, written by make_golden_nb_grad.py) for both methods, a series with no
valid point, a table with none, an empty table, and the argument errors."""
import numpy as np
import pytest
import torch

from conftest import GOLDEN

CASES = ("dense", "masked", "even", "all_masked", "empty", "one_series")


def load_case(name):
    with np.load(GOLDEN / "min_sigma_cases.npz") as z:
        assert tuple(z["cases"]) == CASES
        mask = z[f"{name}:mask"] if f"{name}:mask" in z.files else None
        return z[f"{name}:values"], mask, float(z[f"{name}:global"]), float(z[f"{name}:median"]), z[f"{name}:per_series"]


@pytest.mark.parametrize("name", CASES)
def test_torch_backend_is_the_references_function(name, ftn):
    """The same fp64 numpy operations on the same values: equal to the last bit."""
    tb = ftn.table
    values, mask, want_global, want_median, want_per = load_case(name)
    v = torch.from_numpy(values)
    m = None if mask is None else torch.from_numpy(mask)
    std, per = tb.min_sigma(v, m)
    assert tb._last_backend == "torch" and std.dim() == 0 and std.dtype == per.dtype == torch.float64
    assert float(std) == want_global and per.shape == (values.shape[1],)
    med, per2 = tb.min_sigma(v, m, method="per_series_median")
    assert float(med) == want_median and np.array_equal(per2.numpy(), want_per) and torch.equal(per, per2)


def test_a_series_without_a_valid_point_is_zero_and_outside_the_median(ftn):
    values, mask, _, want_median, want_per = load_case("masked")
    assert (mask[:, 4] == 0).all() and want_per[4] == 0.0 and want_per[6] == 0.0
    med, per = ftn.table.min_sigma(values, mask, method="per_series_median")
    assert float(med) == float(np.median(np.delete(want_per, 4))) == want_median and per[4] == 0


def test_argument_errors(ftn):
    tb = ftn.table
    with pytest.raises(ValueError, match="Unsupported min_sigma_method 'mean'"):
        tb.min_sigma(torch.zeros(4, 2), method="mean")
    with pytest.raises(ValueError, match=r"values must be a \[T, N\] table"):
        tb.min_sigma(torch.zeros(4))
    with pytest.raises(ValueError, match="same shape"):
        tb.min_sigma(torch.zeros(4, 2), torch.ones(4, 3))
    with pytest.raises(ValueError, match="backend 'hip' takes tensors on a ROCm device"):
        tb.min_sigma(torch.zeros(4, 2), backend="hip")


C = 256
RS = [1, 63, 64, 65, C - 1, C, C + 1, 2 * C + 3]
NS = [1, 2, 4, 5, 16, 17, 32, 33, 130]
DS = [8, 24, 64, 96, 128, 136, 512]


@pytest.mark.parametrize("mis", [0, 4, 8, 12])
def test_head_backward_form_table(mis, ftn):
    """Column sums for N <= 4 and a hidden on the 16-byte grid, MFMA tiles otherwise; chunks of 256 rows."""
    rt, lib = ftn.runtime, ftn.lib.load()
    for R in RS:
        for N in NS:
            for D in DS:
                kernel = f"k_headfit_colsum<{N}>" if N <= 4 and mis == 0 else "k_headfit_mfma"
                assert rt.head_backward_form_of(R, N, D, mis) == (kernel, -(-R // C)), (R, N, D)
                assert lib.ftn_head_backward_workspace(R, N, D) == -(-R // C) * 2 * N * (D + 1) * 4


def test_head_backward_chunks_are_capped(ftn):
    """Beyond 256 chunks of 256 rows the chunk grows, to an even number of rows."""
    rt, lib = ftn.runtime, ftn.lib.load()
    assert ftn.lib.FTN_HEADFIT_CHUNKS_MAX == 256
    assert rt.head_backward_form_of(65536, 1, 64) == ("k_headfit_colsum<1>", 256)
    assert rt.head_backward_form_of(65537, 1, 64) == ("k_headfit_colsum<1>", 255)       # chunks of 258 rows
    assert rt.head_backward_form_of(4096 * 96, 5, 64) == ("k_headfit_mfma", 256)
    assert lib.ftn_head_backward_workspace(65537, 1, 64) == 255 * 2 * 65 * 4


@pytest.mark.parametrize("args", [(0, 1, 64, 0), (4, 0, 64, 0), (4, 1, 0, 0), (4, 1, 66, 0), (4, 1, 516, 0),
                                  (4, 1, 64, 3), (4, 1, 64, 16), (1 << 31, 1, 64, 0)])
def test_head_backward_form_rejects_bad_arguments(args, ftn):
    lib = ftn.lib.load()
    assert lib.ftn_head_backward_form(*args) < 0
    assert b"ftn_head_backward_form" in lib.ftn_last_error()
    assert lib.ftn_head_backward_workspace(*args[:3]) == 0 or args[3] != 0


A, M = 0x10000, 0x10004          # stand-ins for device addresses: 16-byte aligned / 4 bytes past a boundary
BWD_GOOD = dict(hidden=A, R=8, N=2, D=8, gr=A, gd=A, sm=A, ss=A, scale=A, wm=A, ws=A, dwm=A, dbm=A, dws=A, dbs=A,
                dh=A, wsp=A, wsb=2 * 2 * 9 * 4)
BWD_BAD = {
    "null hidden": dict(hidden=None), "null g_rate": dict(gr=None), "null sig_sigma": dict(ss=None),
    "null scale": dict(scale=None), "null dW_mu": dict(dwm=None), "null db_sigma": dict(dbs=None),
    "null workspace": dict(wsp=None), "d_hidden without w_mu": dict(wm=None), "R = 0": dict(R=0), "N = 0": dict(N=0),
    "D = 6": dict(D=6), "D = 516": dict(D=516), "g_disp off by 2": dict(gd=A + 2), "d_hidden off by 4": dict(dh=M),
    "w_sigma off by 4 with d_hidden": dict(ws=M), "workspace too small": dict(wsb=2 * 2 * 9 * 4 - 4),
}


@pytest.mark.parametrize("name", list(BWD_BAD))
def test_head_backward_rejects_bad_arguments_before_any_launch(name, ftn):
    lib = ftn.lib.load()
    a = {**BWD_GOOD, **BWD_BAD[name]}
    assert lib.ftn_head_backward_form(8, 2, 8, 0) > 0                  # leaves an earlier message out of the way
    rc = lib.ftn_head_backward(a["hidden"], a["R"], a["N"], a["D"], a["gr"], a["gd"], a["sm"], a["ss"], a["scale"],
                               a["wm"], a["ws"], a["dwm"], a["dbm"], a["dws"], a["dbs"], a["dh"], a["wsp"], a["wsb"],
                               None)
    assert rc < 0 and lib.ftn_last_error().decode().startswith("ftn_head_backward")
    with pytest.raises(ValueError, match="ftn_head_backward"):
        ftn.lib.check(rc, "ftn_head_backward")


FWD_GOOD = dict(hidden=A, rows=8, S=4, D=8, N=2, wm=A, bm=A, ws=A, bs=A, tail=A, tbs=8, hist=4, late=None, lbs=0,
                floor=None, fs=1e-3, rate=A, disp=A, sm=A, ss=A, bad=A)
FWD_BAD = {
    "null hidden": dict(hidden=None), "null sig_mu": dict(sm=None), "null bad": dict(bad=None),
    "rows not a multiple of S": dict(rows=9), "hist = 0": dict(hist=0), "hist > S": dict(hist=5), "N = 0": dict(N=0),
    "D = 6": dict(D=6), "D = 516": dict(D=516), "hidden off by 4": dict(hidden=M), "w_mu off by 4": dict(wm=M),
    "tail off by 2": dict(tail=A + 2), "sig_sigma off by 1": dict(ss=A + 1), "negative tail stride": dict(tbs=-8),
}


@pytest.mark.parametrize("name", list(FWD_BAD))
def test_head_fit_forward_rejects_bad_arguments_before_any_launch(name, ftn):
    lib = ftn.lib.load()
    a = {**FWD_GOOD, **FWD_BAD[name]}
    assert lib.ftn_head_backward_form(8, 2, 8, 0) > 0
    rc = lib.ftn_head_fit_forward(a["hidden"], a["rows"], a["S"], a["D"], a["N"], a["wm"], a["bm"], a["ws"], a["bs"],
                                  a["tail"], a["tbs"], a["hist"], a["late"], a["lbs"], a["floor"], a["fs"], a["rate"],
                                  a["disp"], a["sm"], a["ss"], a["bad"], None)
    assert rc < 0 and lib.ftn_last_error().decode().startswith("ftn_head_fit_forward")


def test_head_wrappers_validate_on_the_host(ftn):
    rt = ftn.runtime
    z = torch.zeros
    with pytest.raises(ValueError, match="hidden must be an fp32 device tensor"):
        rt.head_backward(z(8, 8), z(8, 2), z(8, 2), z(8, 2), z(8, 2), z(1))
    assert {"ftn_head_backward", "ftn_head_backward_form", "ftn_head_backward_workspace",
            "ftn_head_fit_forward"} <= set(ftn.lib.EXPORTS)
