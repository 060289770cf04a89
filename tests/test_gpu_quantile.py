"""NB quantiles and CDF on the MI355X (``ftn_nb_cdf`` / ``ftn_nb_quantiles`` behind ``score.nb_cdf``,
``nb_quantiles``, ``prediction_interval`` and ``interval_metrics``) against the scipy fixtures of
tests/golden/make_golden_quantile.py, which are all these tests read.

CDF accuracy: e = max |F - F_fixture| / max(min(F, 1 - F), 2^-24) per fixture, through the entry's fp64 output (the
fp32 output is checked to be its rounding).  Every case prints ``NBQ_CDF_ERR``.  CDF_BOUND is the 1e-6 that the
quantile rule assumes, for every fixture: the per-fixture figures have not been measured on an MI355X yet (DESIGN.md
section 4, "Quantiles"), and a bound may only be tightened to 4 x a device measurement.  The device arithmetic run
on a CPU (same sources, the hardware reciprocal replaced by one of 3e-8 relative error) gave scalar 2.3e-11, vector
1.0e-10, pipeline 2.4e-11, large 4.9e-11, tiny 2.6e-08.  Quantiles: exact outside near ties
(nbq_checks.check_quantiles)."""
import ctypes as C

import numpy as np
import pytest
import torch

import nbq_checks as nq

pytestmark = pytest.mark.gpu

CDF_BOUND = {name: 1e-6 for name in nq.FIXTURES}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ran(ftn, dev):
    """Every fixture through both kernels, once: name -> (F32, F64, Q, flag) on the host."""
    out = {}
    for name in nq.FIXTURES:
        z = nq.load(name)
        y, rate, disp = (torch.from_numpy(np.array(z[k])).to(dev) for k in ("y", "rate", "disp"))
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        F32, F64 = ftn.runtime.nb_cdf(y, rate, disp, want64=True, flag=flag)
        Q = ftn.score.nb_quantiles(rate, disp, list(z["levels"]))
        assert ftn.score._last_backend == "hip"
        _, qflag = ftn.runtime.nb_quantiles(rate, disp, list(z["levels"]))
        out[name] = (F32.cpu(), F64.cpu(), Q.cpu(), int(flag) | int(qflag))
    return out


@pytest.mark.parametrize("name", nq.FIXTURES)
def test_cdf_accuracy(name, ran):
    assert max(CDF_BOUND.values()) <= 1e-6
    z = nq.load(name)
    F32, F64, _, flag = ran[name]
    e = nq.cdf_error(F64.numpy(), z["F_y"])
    print(f"NBQ_CDF_ERR hip {name} {e:.3e}")
    assert e <= CDF_BOUND[name], (name, e)
    assert flag == 0 and torch.equal(F32, F64.float())


@pytest.mark.parametrize("name", nq.FIXTURES)
def test_quantiles_are_exact(name, ran):
    z = nq.load(name)
    Q = ran[name][2]
    assert Q.dtype == torch.float32
    ties = nq.check_quantiles(Q.numpy(), z, name)
    print(f"NBQ_TIES {name} {ties}/{z['k_star'].size} kmax={float(Q.max()):.0f}")


@pytest.mark.parametrize("name", nq.FIXTURES)
def test_self_consistency(name, ran, ftn, dev):
    """From the kernels alone: F(Q) >= q and F(Q - 1) < q outside the near-tie band, quantiles non-decreasing in the
    level, prediction_interval the same bits as the two rows."""
    z = nq.load(name)
    rate, disp = (torch.from_numpy(np.array(z[k])).to(dev) for k in ("rate", "disp"))
    Q = ran[name][2]
    lv = z["levels"]
    order = np.argsort(lv)
    assert bool((Q[order][1:] >= Q[order][:-1]).all())
    band = nq.band(lv)[:, 0, 0, 0]
    for i, q in enumerate(lv):
        Qi = Q[i].to(dev)
        _, F_at = ftn.runtime.nb_cdf(Qi, rate, disp, want64=True)
        _, F_below = ftn.runtime.nb_cdf(Qi - 1.0, rate, disp, want64=True)
        F_at, F_below, pos = F_at.cpu().numpy(), F_below.cpu().numpy(), (Q[i] > 0).numpy()
        assert bool((F_at >= q - band[i]).all()), (name, q)
        assert bool((F_below[pos] < q + band[i]).all()), (name, q)
    lo, hi = ftn.score.prediction_interval(rate, disp, 0.95)
    if 0.025 in lv and 0.975 in lv:
        assert torch.equal(lo.cpu(), Q[list(lv).index(0.025)]) and torch.equal(hi.cpu(), Q[list(lv).index(0.975)])
    both = ftn.score.nb_quantiles(rate, disp, [0.025, 0.975])
    assert torch.equal(lo, both[0]) and torch.equal(hi, both[1])


def test_forms(ftn, dev, ran):
    rt = ftn.runtime
    for name in nq.FIXTURES:
        z = nq.load(name)
        y, rate, disp = (torch.from_numpy(np.array(z[k])).to(dev) for k in ("y", "rate", "disp"))
        want = "vec4" if z["rate"].shape[2] % 4 == 0 else "scalar"
        assert (want == "vec4") == (name in ("vector", "large", "tiny"))
        assert rt.nbq_form(rate, disp) == want and rt.nbq_form(rate, disp, y) == want, name
    z = nq.load("vector")
    B, H, N = z["rate"].shape
    y, rate, disp = (torch.from_numpy(np.array(z[k])).to(dev) for k in ("y", "rate", "disp"))
    levels = list(z["levels"])
    wide = torch.zeros(B, H * N + 2, device=dev)
    wide[:, :H * N] = rate.reshape(B, -1)
    strided = wide[:, :H * N].view(B, H, N)
    buf = torch.zeros(B * H * N + 1, device=dev)
    buf[1:] = rate.reshape(-1)
    offset = buf[1:].view(B, H, N)
    assert strided.stride(0) == H * N + 2 and offset.data_ptr() % 16 == 4
    for view in (strided, offset):
        assert rt.nbq_form(view, disp) == "scalar" and rt.nbq_form(view, disp, y) == "scalar"
        Q, _ = rt.nb_quantiles(view, disp, levels)
        assert torch.equal(Q.cpu(), ran["vector"][2])
        F32, F64 = rt.nb_cdf(y, view, disp, want64=True)
        assert torch.equal(F32.cpu(), ran["vector"][0]) and torch.equal(F64.cpu(), ran["vector"][1])
    wide4 = torch.zeros(B, H * N + 4, device=dev)
    wide4[:, :H * N] = rate.reshape(B, -1)
    v4 = wide4[:, :H * N].view(B, H, N)
    assert rt.nbq_form(v4, disp) == "vec4"
    assert torch.equal(rt.nb_quantiles(v4, disp, levels)[0].cpu(), ran["vector"][2])


def test_edges(ftn, dev):
    sc, rt = ftn.score, ftn.runtime
    z = nq.load("vector")
    y, rate, disp = (torch.from_numpy(np.array(z[k])).to(dev) for k in ("y", "rate", "disp"))
    levels = [0.1, 0.9]
    base, _ = rt.nb_quantiles(rate, disp, levels)
    Fbase = sc.nb_cdf(y, rate, disp)
    r2, d2 = rate.clone(), disp.clone()
    bad = torch.zeros(rate.shape, dtype=torch.bool, device=dev)
    r2[0, 1, 2], d2[1, 3, 4], r2[2, 5, 6], d2[3, 7, 9] = float("nan"), float("inf"), float("inf"), float("nan")
    bad[0, 1, 2] = bad[1, 3, 4] = bad[2, 5, 6] = bad[3, 7, 9] = True
    Q, flag = rt.nb_quantiles(r2, d2, levels)
    assert int(flag) == 0 and bool(torch.isnan(Q[:, bad]).all()) and torch.equal(Q[:, ~bad], base[:, ~bad])
    cflag = torch.zeros(1, dtype=torch.int32, device=dev)
    y2 = y.clone()
    y2[0, 0, 5] = float("nan")
    F = rt.nb_cdf(y2, r2, d2, flag=cflag)
    bad_y = bad.clone()
    bad_y[0, 0, 5] = True
    assert int(cflag) == 0 and bool(torch.isnan(F[bad_y]).all()) and torch.equal(F[~bad_y], Fbase[~bad_y])
    # below eps = eps
    small, eps = torch.full_like(rate, 1e-12), torch.full_like(rate, 1e-8)
    assert torch.equal(sc.nb_quantiles(small, disp, [0.5]), sc.nb_quantiles(eps, disp, [0.5]))
    assert torch.equal(sc.nb_quantiles(torch.zeros_like(rate), disp, [0.5]), sc.nb_quantiles(eps, disp, [0.5]))
    assert torch.equal(sc.nb_cdf(y, rate, small), sc.nb_cdf(y, rate, eps))
    assert torch.equal(sc.nb_cdf(y, -rate, disp), sc.nb_cdf(y, eps, disp))
    # y < 0 = 0, fractional y = floor(y)
    assert torch.equal(sc.nb_cdf(torch.full_like(y, -2.0), rate, disp), sc.nb_cdf(torch.zeros_like(y), rate, disp))
    yy = torch.floor(y.clamp(min=0.0))
    assert torch.equal(sc.nb_cdf(yy + 0.5, rate, disp), sc.nb_cdf(yy, rate, disp))
    # an answer beyond 2^24: NaN at that element alone, bit 1 of the flag, check=True raises
    r3 = rate.clone()
    r3[1, 1, 1] = 1e8
    Q, flag = rt.nb_quantiles(r3, disp, [0.5, 0.1])
    assert int(flag) == ftn.lib.FTN_NBQ_RANGE == 2
    assert bool(torch.isnan(Q[:, 1, 1, 1]).all()) and int(torch.isnan(Q).sum()) == 2
    with pytest.raises(ValueError, match="2\\^24"):
        sc.nb_quantiles(r3, disp, [0.5], check=True)
    assert bool(torch.isfinite(sc.nb_quantiles(rate, disp, [0.5], check=True)).all())
    y3 = y.clone()
    y3[2, 2, 2] = 3e7
    F = rt.nb_cdf(y3, rate, disp, flag=cflag)
    assert int(cflag) == 2 and bool(torch.isnan(F[2, 2, 2])) and int(torch.isnan(F).sum()) == 1


def test_nine_levels_are_two_chunks(ftn, dev):
    sc = ftn.score
    z = nq.load("scalar")
    rate, disp = (torch.from_numpy(np.array(z[k])).to(dev) for k in ("rate", "disp"))
    nine = [0.9, 0.025, 0.5, 0.975, 0.1, 0.3, 0.7, 0.05, 0.95]
    Q8, Q9 = sc.nb_quantiles(rate, disp, nine[:8]), sc.nb_quantiles(rate, disp, nine)
    assert tuple(Q9.shape) == (9,) + tuple(rate.shape) and torch.equal(Q9[:8], Q8)
    assert torch.equal(Q9[8], sc.nb_quantiles(rate, disp, [0.95])[0])
    for q, row in zip(z["levels"], z["k_star"]):
        assert np.array_equal(Q9[nine.index(float(q))].cpu().numpy().astype(np.float64), row)


def test_c_entry_rejects_bad_arguments(ftn, dev):
    lib = ftn.lib.load()
    rate = torch.ones(2, 3, 4, device=dev)
    out = torch.empty(9, 2, 3, 4, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream

    def call(levels, Q, r=rate.data_ptr(), o=out.data_ptr(), f=flag.data_ptr(), lv_null=False):
        arr = (C.c_double * 9)(*levels, *([0.5] * (9 - len(levels))))
        return lib.ftn_nb_quantiles(r, 12, rate.data_ptr(), 12, 2, 3, 4, None if lv_null else arr, Q, 1e-8, o, f, st)

    assert call([0.5], 1) == 0
    assert call([0.5], 0) < 0 and call([0.5] * 9, 9) < 0
    assert call([0.0], 1) < 0 and call([0.5, 1.0], 2) < 0
    assert call([0.5], 1, r=None) < 0 and call([0.5], 1, o=None) < 0 and call([0.5], 1, f=None) < 0
    assert call([0.5], 1, lv_null=True) < 0
    assert b"ftn_nb_quantiles" in lib.ftn_last_error()
    p = rate.data_ptr()
    assert lib.ftn_nb_cdf(None, 12, p, 12, p, 12, 2, 3, 4, 1e-8, out.data_ptr(), None, None, st) < 0
    assert lib.ftn_nb_cdf(p, 12, p, 12, p, 12, 2, 0, 4, 1e-8, out.data_ptr(), None, None, st) < 0
    assert lib.ftn_nb_cdf(p, 12, p, 12, p, 12, 2, 3, 4, 1e-8, out.data_ptr(), None, None, st) == 0
    torch.cuda.synchronize()
    assert int(flag) == 0


def test_model_forward_feeds_the_intervals_without_a_synchronisation(ftn, dev):
    """rate, disp = model(x) on the device -> prediction_interval and interval_metrics; nothing synchronises until
    the test reads (torch's sync debug mode raises on any synchronising call)."""
    sc = ftn.score
    L, H, N, B = 24, 6, 24, 4
    cfg = dict(input_len=L, pred_len=H, d_model=16, d_ff=32, n_layers=2, k_periods=3, kernel_set=[(3, 3), (5, 5)],
               dropout=0.0, activation="gelu", mode="direct", use_checkpoint=False)
    g = torch.Generator().manual_seed(1)
    torch.manual_seed(0)
    model = ftn.models.TimesNet(**cfg).eval()
    with torch.no_grad():
        model(torch.rand(2, L, N, generator=g) + 1.0)
        for p in model.parameters():
            if float(p.abs().sum()) == 0.0:
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
    model = model.to(dev)
    t = torch.arange(L, dtype=torch.float32).view(1, L, 1)
    x = (torch.rand(B, L, N, generator=g) + 1.5 + torch.sin(2 * torch.pi * t / 6.0)).to(dev)
    yb = torch.poisson(torch.full((B, H, N), 2.0), generator=g).to(dev)
    levels = [0.05, 0.5, 0.95]
    with torch.inference_mode():
        rate, disp = model(x)
        sc.interval_metrics(yb, rate, disp, levels)             # warm-up: allocator, library load
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            lo, hi = sc.prediction_interval(rate, disp, 0.9)
            assert sc._last_backend == "hip"
            met = sc.interval_metrics(yb, rate, disp, levels)
            ev = torch.cuda.Event()
            ev.record()
            done_at_once = ev.query()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    assert isinstance(done_at_once, bool) and all(v.is_cuda for v in met.values())
    ev.synchronize()
    Q = sc.nb_quantiles(rate, disp, levels, check=True)
    assert torch.equal(lo, Q[0]) and torch.equal(hi, Q[2]) and bool((lo <= hi).all())
    want = sc.interval_metrics(yb.cpu(), rate.cpu(), disp.cpu(), levels)
    assert sc._last_backend == "torch"
    n = yb.numel()
    assert int(met["count"]) == int(want["count"]) == n
    # the backends agree on every quantile here unless a near tie separates them; the means are fp32 sums of n terms
    assert float((met["coverage"].cpu() - want["coverage"]).abs().max()) <= 1.0 / n + 2 * nq.U32
    assert float((met["pinball"].cpu() - want["pinball"]).abs().max()) <= 1.0 / n + n * 2.0 ** -23
    assert abs(float(met["pit_mean"]) - float(want["pit_mean"])) <= n * 2.0 ** -23


@pytest.mark.parametrize("name", ["scalar", "vector"])
def test_interval_metrics_against_numpy(name, ftn, dev):
    """Coverage is a ratio of counts (exact in fp32 up to the one division, and off by 1 / n per near tie at most);
    pinball and mean PIT are fp32 sums of n terms of one sign: relative error <= n 2^-24 for any summation order,
    asserted as n 2^-23 (times the mean for pinball; PIT terms are <= 1), plus the fp32 rounding of F itself."""
    sc = ftn.score
    z = nq.load(name)
    y, rate, disp = (torch.from_numpy(np.array(z[k])).to(dev) for k in ("y", "rate", "disp"))
    mask = (torch.rand(y.shape, generator=torch.Generator().manual_seed(0)) >= 0.2)
    lvb = z["levels"].reshape(-1, 1, 1, 1)
    tied = (np.abs(z["F_k"] - lvb) <= nq.band(z["levels"])) | (np.abs(z["F_km1"] - lvb) <= nq.band(z["levels"]))
    for m in (None, mask):
        got = {k: v.cpu() for k, v in sc.interval_metrics(y, rate, disp, list(z["levels"]),
                                                          None if m is None else m.to(dev)).items()}
        assert sc._last_backend == "hip"
        valid = np.ones(y.shape, bool) if m is None else m.numpy()
        cov, pin, pit = nq.interval_metrics_numpy(z, valid)
        n = int(valid.sum())
        assert int(got["count"]) == n
        ties = (tied & valid).sum((1, 2, 3))
        cerr = np.abs(got["coverage"].numpy() - cov)
        assert np.all(cerr[ties == 0] <= 2 * nq.U32) and np.all(cerr <= ties / n + 2 * nq.U32), (cerr, ties)
        tol = n * 2.0 ** -23
        assert np.all(np.abs(got["pinball"].numpy() - pin) <= tol * np.maximum(pin, 1.0) + ties / n)
        assert abs(float(got["pit_mean"]) - pit) <= tol + nq.U32


def test_poisson_limit_is_finite_and_near_poisson(ftn, dev):
    """Dispersion at the clamp (alpha = 1e-8, r = 1e8): supported, but scipy's own accuracy there was not examined, so
    the only claim is finite outputs within 1 of scipy.stats.poisson.ppf (stored by the generator)."""
    with np.load(nq.GOLDEN / "nbq_poisson.npz") as z:
        rate, disp, lv, ppf = (np.array(z[k]) for k in ("rate", "disp", "levels", "ppf"))
    r, d = torch.from_numpy(rate).to(dev), torch.from_numpy(disp).to(dev)
    Q, flag = ftn.runtime.nb_quantiles(r, d, list(lv))
    F = ftn.score.nb_cdf(Q[2], r, d)
    assert int(flag) == 0 and bool(torch.isfinite(Q).all()) and bool(torch.isfinite(F).all())
    assert float(np.abs(Q.cpu().numpy().astype(np.float64) - ppf).max()) <= 1.0
    Q0, _ = ftn.runtime.nb_quantiles(r, torch.zeros_like(d), list(lv))
    assert torch.equal(Q0, Q)
