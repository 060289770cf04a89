"""Table preparation on the GPU: the HIP backend of ``table`` (csrc/table.hip) against the reference's outputs
(tests/golden/table_cases.npz), against an fp64 restatement with the rounding points of include/flowtimes.h
(tests/table_checks.py) over the shape sweep, and against the torch backend bit for bit where the arithmetic is
elementwise.  Every test asserts that the HIP backend ran.

Bounds, from the roundings (none is taken from what the kernels give):

* ``mean``: the fp64 sum is rounded to fp32 once.  The restatement adds in another order; two fp64 sums of at most
  65536 fp32 terms differ by far less than an fp32 half-spacing, so the two roundings agree except at a tie:
  MEAN_ULPS = 1.
* ``std``, ``diff_std`` and the scaler's std, given the same fp32 mean: css / count is rounded to fp32 once (half a
  spacing), the square root halves a relative error and is itself rounded once (half a spacing): each side is within
  0.75 spacings of the exact value, the two sides within 1.5: STD_ULPS = 2.  The restatement is therefore evaluated
  at the mean the kernel reports (asserted to be within MEAN_ULPS of the restated one).
* against the reference: its own distance from the restatement on the same table, plus the bound above.
* ``seasonal_strength``: the project's rtol 1e-4; every bin of ``power_out`` within 1e-4 of the column's fp64 peak
  power; the chosen bin holds at least (1 - 1e-4) of the fp64 maximum.
* ``transform`` and ``inverse``: equal bits (one rounding per operation on both sides)."""
import numpy as np
import pytest
import torch

import table_checks as tc

pytestmark = pytest.mark.gpu
DEV = "cuda"
MEAN_ULPS, STD_ULPS = 1, 2
POISON = 0x7FA5A5A5                                             # a NaN whose payload is recognisable


@pytest.fixture(scope="module")
def fx():
    return tc.fixture()


def carve(n, dtype, shape=None, pad=24):
    """A tensor of ``n`` elements inside a poisoned buffer, and the check that its surroundings were left alone."""
    words = 2 if dtype == torch.float64 else 1
    raw = torch.full(((n + 2 * pad) * words,), POISON, dtype=torch.int32, device=DEV)
    buf = raw.view(dtype)
    out = buf[pad:pad + n]
    out = out.view(shape) if shape is not None else out

    def untouched():
        r = raw.view(-1, words)
        return bool((r[:pad] == POISON).all()) and bool((r[pad + n:] == POISON).all())
    return out, untouched


def run_hip(ftn, X, M, power=False):
    """The pieces behind ``series_features`` with every output carved from a poisoned buffer:
    ``(features, stats, f_peak, peak, total, power or None)`` as numpy."""
    rt = ftn.runtime
    T, N = X.shape
    checks = []
    stats, c = carve(12 * N, torch.float64, (12, N)); checks.append(c)
    rt.table_moments(X, M, diffs=True, out=stats)
    fp, c = carve(N, torch.int32); checks.append(c)
    pk, c = carve(N, torch.float32); checks.append(c)
    tt, c = carve(N, torch.float32); checks.append(c)
    pw = None
    if power and T >= 2:
        pw, c = carve((T // 2) * N, torch.float32, (T // 2, N)); checks.append(c)
    rt.table_spectrum(X, stats[2].to(torch.float32), M, power_out=pw, outs=(fp, pk, tt))
    ft, c = carve(5 * N, torch.float32, (N, 5)); checks.append(c)
    rt.table_features(stats, fp, pk, tt, T, out=ft)
    torch.cuda.synchronize()
    assert all(c() for c in checks), "bytes around an output were written"
    whole = ftn.table.series_features(X, M)
    assert ftn.table._last_backend == "hip" and tc.same_bits(whole, ft)
    return tuple(None if t is None else t.cpu().numpy() for t in (ft, stats, fp, pk, tt, pw))


def check_against_restatement(X, M, feats, stats, f_peak, power, tag):
    """The five features of one table against the fp64 restatement; returns the restated features."""
    T, N = X.shape
    base, _ = tc.features64(X, M)
    assert tc.ulps(feats[:, 0], base[:, 0]).max() <= MEAN_ULPS, (tag, "mean")
    dmean = stats[8].astype(np.float32) if T > 1 else None
    if T > 1:
        dx, ok = tc.diffs_of(X, M)
        assert tc.ulps(dmean, tc.moments64(dx, ok)["mean"]).max() <= MEAN_ULPS, (tag, "diff mean")
    want, P = tc.features64(X, M, mean32=feats[:, 0], dmean32=dmean)
    assert tc.ulps(feats[:, 1], want[:, 1]).max() <= STD_ULPS, (tag, "std", tc.ulps(feats[:, 1], want[:, 1]).max())
    assert tc.ulps(feats[:, 2], want[:, 2]).max() <= STD_ULPS, (tag, "diff_std", tc.ulps(feats[:, 2], want[:, 2]).max())
    if T == 1:
        assert not feats[:, 2:].any() and not f_peak.any()
        return want
    top = P.max(axis=0)
    if power is not None:
        assert power.shape == P.shape
        err = np.abs(power.astype(np.float64) - P).max(axis=0)
        print(tag, "max bin error / peak", float((err / np.maximum(top, 1e-300)).max()))
        assert (err <= 1e-4 * top).all(), (tag, "power_out", float((err / np.maximum(top, 1e-300)).max()))
    assert ((f_peak >= 1) & (f_peak <= T // 2)).all(), (tag, "f_peak range")
    chosen = P[f_peak - 1, np.arange(N)]
    assert (chosen >= (1 - 1e-4) * top).all(), (tag, "chosen bin")
    rel = np.abs(feats[:, 3].astype(np.float64) - want[:, 3]) / np.maximum(np.abs(want[:, 3].astype(np.float64)), 1e-300)
    print(tag, "seasonal_strength max rel", float(np.where(want[:, 3] == feats[:, 3], 0, rel).max()))
    assert np.allclose(feats[:, 3], want[:, 3], rtol=1e-4, atol=0), (tag, "seasonal_strength")
    tot = P.sum(axis=0)
    live = tot.astype(np.float32) > np.float32(1e-6)
    assert (feats[:, 4] == np.where(live, (float(T) / f_peak).astype(np.float32), 0)).all(), (tag, "dominant_period")
    return want


# ---------------------------------------------------------------- fixtures
@pytest.mark.parametrize("name", ["planted", "mixed", "neg", "t1", "t2", "t3"])
def test_features_on_the_fixtures(name, ftn, fx):
    meta, arrays = fx
    X, M, ref = arrays[f"{name}:X"], arrays[f"{name}:M"], arrays[f"{name}:features"]
    feats, stats, f_peak, peak, total, power = run_hip(ftn, torch.from_numpy(X).to(DEV), torch.from_numpy(M).to(DEV), True)
    want = check_against_restatement(X, M, feats, stats, f_peak, power, name)
    assert tc.same_bits(torch.from_numpy(feats[:, 4]), torch.from_numpy(ref[:, 4])), "dominant_period"
    assert np.allclose(feats[:, 3], ref[:, 3], rtol=1e-4, atol=0), "seasonal_strength against the reference"
    base, _ = tc.features64(X, M)
    for k, bound in ((0, MEAN_ULPS), (1, STD_ULPS), (2, STD_ULPS)):
        own = tc.ulps(ref[:, k], base[:, k])                    # the reference's distance from the restatement
        print(name, tc.FEATURES[k], "reference is off by", own.max(), "spacings; hip by", tc.ulps(feats[:, k], base[:, k]).max())
        assert (tc.ulps(feats[:, k], ref[:, k]) <= own + bound + (MEAN_ULPS if k else 0)).all(), (name, tc.FEATURES[k])


@pytest.mark.parametrize("name", ["planted", "mixed", "neg", "t2"])
def test_scaler_on_the_fixtures(name, ftn, fx):
    meta, arrays = fx
    m = meta["tables"][name]
    Xh = arrays[f"{name}:X"]
    X = torch.from_numpy(Xh).to(DEV)
    (a0, a1), (v0, v1) = m["train"], m["val"]
    pred = torch.from_numpy(arrays[f"{name}:pred"]).to(DEV)
    for method, per_series in tc.FITS:
        key = tc.fit_key(name, method, per_series)
        ref = arrays[f"{key}:pairs"]
        sc = ftn.table.SeriesScaler.fit(X[a0:a1], method, per_series=per_series, clip_negative=m["clip"])
        assert ftn.table._last_backend == "hip" and sc.loc.device.type == "cuda"
        got = sc.pairs()
        want = tc.pairs64(Xh[a0:a1], method, per_series, clip=m["clip"])
        if method == "minmax":
            assert np.array_equal(got, ref) and np.array_equal(got, want), key
        else:
            assert tc.ulps(got[:, 0], want[:, 0]).max() <= MEAN_ULPS, key
            # the std at the mean the kernel reports: per series the restatement takes it; the global pair is centred
            # in fp64 throughout, so one spacing of the mean moves css by n (dm)^2, far below a spacing of the std
            assert tc.ulps(got[:, 1], want[:, 1]).max() <= STD_ULPS + MEAN_ULPS, (key, tc.ulps(got[:, 1], want[:, 1]).max())
            for k in (0, 1):
                own = tc.ulps(ref[:, k], want[:, k])
                assert (tc.ulps(got[:, k], ref[:, k]) <= own + STD_ULPS + MEAN_ULPS).all(), key
        # the eps rule ran on the device: a column that is constant below eps divides by 1
        if name == "mixed" and per_series:
            assert sc.scale[[2, 6, 7]].tolist() == [1.0, 1.0, 1.0] and bool((sc.scale > 0).all())
        # given the reference's pairs, transform and inverse are the reference's arrays
        if f"{key}:val" not in arrays:                          # the large table's global fits: pairs only
            assert name == "planted" and not per_series
            continue
        ld = ftn.table.SeriesScaler.from_pairs(method, ref, device=DEV)
        out, ok = carve((v1 - v0) * Xh.shape[1], torch.float32, (v1 - v0, Xh.shape[1]))
        assert ld.transform(X[v0:v1], out=out, clip_negative=m["clip"]) is out and ftn.table._last_backend == "hip"
        assert torch.equal(out.cpu(), torch.from_numpy(arrays[f"{key}:val"])) and ok(), key
        assert torch.equal(ld.inverse(pred).cpu(), torch.from_numpy(arrays[f"{key}:inv"])), key
        assert ftn.table._last_backend == "hip"
        # and the torch backend gives the same bits on the same device tensors
        assert tc.same_bits(ld.transform(X[v0:v1], clip_negative=m["clip"], backend="torch"), out)
        assert tc.same_bits(ld.inverse(pred, backend="torch"), ld.inverse(pred))


# ---------------------------------------------------------------- sweep
@pytest.mark.parametrize("case", tc.sweep(), ids=tc.case_id)
def test_sweep_against_fp64(case, ftn):
    Xh, Mh = tc.sweep_table(case)
    X = tc.place(Xh, case["layout"], DEV)
    M = None if Mh is None else tc.place(Mh, case["layout"], DEV)
    kw = tc.layout_args(case)
    rt = ftn.runtime
    assert rt.table_moments(X, M, diffs=True, form=True) == tc.want_moments_form(case["T"], case["N"], mask=M is not None, **kw)
    assert rt.table_spectrum(X, None, M, form=True) == tc.want_spectrum_form(case["T"], case["N"], has_mask=M is not None, **kw)
    tag = f"T{case['T']} N{case['N']} {case['mask']} {case['layout']}"
    feats, stats, f_peak, peak, total, power = run_hip(ftn, X, M, True)
    check_against_restatement(Xh, Mh, feats, stats, f_peak, power, tag)
    if case["mask"] == "column" and case["T"] > 1:
        assert feats[0].tolist() == [0, 0, 0, 0, 0] and f_peak[0] == 1
    # the scaler of the same table in the same layout: all four fits at the restatement
    for method, per_series in tc.FITS:
        got = ftn.table.SeriesScaler.fit(X, method, per_series=per_series).pairs()
        want = tc.pairs64(Xh, method, per_series)
        assert ftn.table._last_backend == "hip"
        assert tc.ulps(got[:, 0], want[:, 0]).max() <= MEAN_ULPS, (tag, method, per_series)
        assert tc.ulps(got[:, 1], want[:, 1]).max() <= STD_ULPS + MEAN_ULPS, (tag, method, per_series)
    # transform in place of the layout: equal bits to the torch backend, the table's surroundings untouched
    sc = ftn.table.SeriesScaler.fit(X, "zscore")
    want = sc.transform(X, backend="torch")
    assert rt.table_affine(X, sc.loc, sc.scale, form=True)["load_bytes"] == tc.want_affine_form(
        case["T"], case["N"], 1, x_strides=(X.stride(0) if case["T"] > 1 else case["N"], 1),
        misalign={"x": X.data_ptr() % 16}, o_strides=(case["N"], 1))["load_bytes"]
    assert tc.same_bits(sc.transform(X), want) and ftn.table._last_backend == "hip"
    Y = X.clone() if case["layout"] == "dense" else X
    if case["layout"] == "slice4" and case["N"] % 4 == 0 and case["T"] > 1:     # four series a lane over a row stride > N
        assert rt.table_affine(Y, sc.loc, sc.scale, out=Y, form=True)["lane_axis"] == 2 and Y.stride(0) == case["N"] + 8
    assert sc.transform(Y, out=Y) is Y and tc.same_bits(Y.contiguous(), want)
    if case["layout"] in ("slice", "slice4"):                   # the wider table's other columns keep their NaNs
        big, c0 = X._base, X.storage_offset()
        assert big.shape == (case["T"], case["N"] + 8) and c0 in (3, 4)
        assert bool(torch.isnan(big[:, :c0]).all()) and bool(torch.isnan(big[:, c0 + case["N"]:]).all())


def test_white_noise_hits_the_reference_bin(ftn):
    """T = 731, N = 512 white noise: the smallest top-two gap of this seed is 1.76e-3 relative (fp64), far above the
    kernel's error, so the bin must be pocketfft's (the torch backend is the reference's numpy)."""
    g = np.random.default_rng(732)
    Xh = g.standard_normal((731, 512)).astype(np.float32)
    ref = ftn.table.series_features(torch.from_numpy(Xh))
    assert ftn.table._last_backend == "torch"
    got = ftn.table.series_features(torch.from_numpy(Xh).to(DEV))
    assert ftn.table._last_backend == "hip"
    assert tc.same_bits(got[:, 4].cpu(), ref[:, 4])
    assert torch.allclose(got[:, 3].cpu(), ref[:, 3], rtol=1e-4, atol=0)


# ---------------------------------------------------------------- edge rows
def test_non_finite_values_and_the_mask(ftn):
    g = np.random.default_rng(9)
    Xh = g.poisson(6.0, size=(66, 9)).astype(np.float32)
    Mh = np.ones_like(Xh)
    Mh[5, 2] = Mh[40, 7] = 0.0
    X, M = torch.from_numpy(Xh).to(DEV), torch.from_numpy(Mh).to(DEV)
    clean = ftn.table.series_features(X, M)
    assert ftn.table._last_backend == "hip"
    # a NaN under a zero mask changes nothing (the reference would poison the column: DESIGN.md section 8)
    Xn = X.clone()
    Xn[5, 2], Xn[40, 7] = float("nan"), float("inf")
    assert tc.same_bits(ftn.table.series_features(Xn, M), clean)
    # a NaN and an inf inside the mask of column 4: the stated five values, the other columns keep their bits
    Xb = X.clone()
    Xb[7, 4], Xb[30, 4] = float("nan"), float("inf")
    bad = ftn.table.series_features(Xb, M).cpu()
    assert torch.isnan(bad[4, :4]).all() and bad[4, 4] == 0
    keep = [c for c in range(9) if c != 4]
    assert tc.same_bits(bad[keep], clean.cpu()[keep])
    without = ftn.table.series_features(X[:, keep], M[:, keep])
    assert tc.same_bits(without, clean[keep])
    Xi = X.clone()
    Xi[30, 4] = float("inf")                                    # an inf alone: the same five values
    lone = ftn.table.series_features(Xi, M).cpu()
    assert torch.isnan(lone[4, :4]).all() and lone[4, 4] == 0 and tc.same_bits(lone[keep], clean.cpu()[keep])
    # two runs are bit-identical
    assert tc.same_bits(ftn.table.series_features(X, M), clean)
    assert tc.same_bits(ftn.table.series_features(Xb, M).cpu(), bad)


def test_negative_zero_clip_and_constant_columns(ftn):
    g = np.random.default_rng(10)
    Xh = (g.standard_normal((45, 8)) * 3).astype(np.float32)
    Xh[:, 3] = 2.5                                              # constant
    Xh[:, 5] = -1.0                                             # constant, and 0 once clipped
    Xh[4, 0] = -0.0
    X = torch.from_numpy(Xh).to(DEV)
    for method, per_series in tc.FITS:
        for clip in (False, True):
            sc = ftn.table.SeriesScaler.fit(X, method, per_series=per_series, clip_negative=clip)
            assert ftn.table._last_backend == "hip"
            ref = ftn.table.SeriesScaler.fit(torch.from_numpy(Xh), method, per_series=per_series, clip_negative=clip)
            want = tc.pairs64(Xh, method, per_series, clip=clip)
            got = sc.pairs()
            assert tc.ulps(got[:, 0], want[:, 0]).max() <= MEAN_ULPS and tc.ulps(got[:, 1], want[:, 1]).max() <= STD_ULPS + MEAN_ULPS
            if per_series:
                assert sc.scale[3].item() == 1.0 and sc.scale[5].item() == 1.0          # a constant column: scale 1
            if method == "minmax":
                assert np.array_equal(got, ref.pairs())
            t_hip = sc.transform(X, clip_negative=clip)
            assert tc.same_bits(t_hip, sc.transform(X, clip_negative=clip, backend="torch"))
            if clip:                                            # the clipped table is never materialised
                assert torch.equal(X.cpu(), torch.from_numpy(Xh))
                assert tc.same_bits(t_hip, sc.transform(torch.where(X < 0, torch.zeros_like(X), X)))
    # -0 passes the inverse's clip as it is on both backends (r < 0 ? 0 : r), and compares equal to numpy's +0
    one = ftn.table.SeriesScaler.from_pairs("zscore", np.array([[0.0, 1.0]] * 8), device=DEV)
    z = torch.tensor([[-0.0, 0.0, -1.0, 1.0, float("nan"), float("inf"), -float("inf"), 2.5]], device=DEV)
    got = one.inverse(z)
    assert tc.same_bits(got, one.inverse(z, backend="torch"))
    assert got[0, 2].item() == 0 and got[0, 6].item() == 0 and torch.isnan(got[0, 4]) and got[0, 7].item() == 2.5


# ---------------------------------------------------------------- inverse
def test_inverse_layouts_against_the_torch_backend(ftn):
    g = np.random.default_rng(11)
    Ncols = 211
    pairs = np.stack([g.uniform(-2, 30, Ncols), g.uniform(0.1, 9, Ncols)], axis=1)
    sc = ftn.table.SeriesScaler.from_pairs("zscore", pairs, device=DEV)
    rt = ftn.runtime

    def both(x, **kw):
        want = sc.inverse(x, backend="torch", **kw)
        got = sc.inverse(x, **kw)
        assert ftn.table._last_backend == "hip" and tc.same_bits(got, want), (tuple(x.shape), kw.keys())
        return want

    for P, B, H in ((3, 193, 28), (2, 65, 7), (1, 4, 1)):
        ids = torch.from_numpy(g.integers(0, Ncols, B)).to(DEV)                 # repeated and out of order
        ids[0], ids[-1] = Ncols - 1, 0
        x = torch.from_numpy(g.standard_normal((P, B, H, 1)).astype(np.float32) * 3).to(DEV)
        want = both(x, axis=1, series=ids)
        both(x[0], axis=0, series=ids)                                          # [B, H, 1]
        both(x, axis=1, series=ids, clip=False)
        big = torch.from_numpy(g.standard_normal((P, B, H + 5, 1)).astype(np.float32)).to(DEV)
        both(big[:, :, 2:2 + H], axis=1, series=ids)                            # strided along the series and outer axes
        both(x.permute(1, 0, 2, 3), axis=0, series=ids)                         # no single outer stride: copied
        if H % 4 == 0:                                          # an aligned strided view: 16-byte lanes of one series
            wide = torch.from_numpy(g.standard_normal((P, B, H + 8, 1)).astype(np.float32)).to(DEV)
            v = wide[:, :, 4:4 + H]
            f = rt.table_affine(v, sc.loc, sc.inv_scale, axis=1, series=ids, inverse=True, out=v, form=True)
            assert f["lane_axis"] == 1 and f["load_bytes"] == 16 and v.stride(1) == H + 8
            vw = both(v, axis=1, series=ids)
            keep = wide.clone()
            assert sc.inverse(v, axis=1, series=ids, out=v) is v and tc.same_bits(v.contiguous(), vw)
            assert tc.same_bits(wide[:, :, :4], keep[:, :, :4]) and tc.same_bits(wide[:, :, 4 + H:], keep[:, :, 4 + H:])
        buf = x.clone()                                                         # out= aliasing the input
        assert sc.inverse(buf, axis=1, series=ids, out=buf) is buf and tc.same_bits(buf, want)
        out, ok = carve(x.numel(), torch.float32, tuple(x.shape))
        sc.inverse(x, axis=1, series=ids, out=out)
        torch.cuda.synchronize()
        assert ok() and tc.same_bits(out, want)
        f = rt.table_affine(x, sc.loc, sc.inv_scale, axis=1, series=ids, inverse=True, form=True)
        assert f["lane_axis"] == tc.want_affine_form(P, B, H)["lane_axis"]
    for B, H, N in ((5, 28, Ncols), (3, 7, 64), (2, 3, 1)):
        x = torch.from_numpy(g.standard_normal((B, H, N)).astype(np.float32) * 3).to(DEV)
        cols = torch.from_numpy(g.permutation(Ncols)[:N].copy()).to(DEV)
        both(x, series=cols)                                                    # [B, H, N], series last
        both(x[:, 1:], series=cols, clip=False)
        if N % 4 == 0:                                          # an aligned column slice: 16-byte lanes of four series
            wide = torch.from_numpy(g.standard_normal((B, H, N + 8)).astype(np.float32)).to(DEV)
            v = wide[:, :, 4:4 + N]
            f = rt.table_affine(v, sc.loc, sc.inv_scale, series=cols, inverse=True, out=v, form=True)
            assert f["lane_axis"] == 2 and f["load_bytes"] == 16 and v.stride(1) == N + 8
            vw = both(v, series=cols)
            keep = wide.clone()
            assert sc.inverse(v, series=cols, out=v) is v and tc.same_bits(v.contiguous(), vw)
            assert tc.same_bits(wide[:, :, :4], keep[:, :, :4]) and tc.same_bits(wide[:, :, 4 + N:], keep[:, :, 4 + N:])
        if N == Ncols:
            both(x)
            both(x[:, 1:], clip=False)
    with pytest.raises(ValueError, match="cannot be walked"):
        x = torch.zeros(4, 6, 8, device=DEV)
        sc.inverse(x, axis=1, series=torch.zeros(6, dtype=torch.int64), out=torch.zeros(8, 6, 4, device=DEV).permute(2, 1, 0))


# ---------------------------------------------------------------- one realistic shape
def test_realistic_shape(ftn):
    T, N = 1913, 512
    g = np.random.default_rng(1913)
    t = np.arange(T)[:, None]
    rate = g.uniform(1, 50, (1, N)) * (1 + 0.5 * np.sin(2 * np.pi * t / 7 + g.uniform(0, 6, (1, N)))
                                       + 0.2 * np.sin(2 * np.pi * t / 365.25 + g.uniform(0, 6, (1, N))))
    Xh = g.poisson(rate).astype(np.float32)
    Mh = (g.random((T, N)) >= 0.1).astype(np.float32)
    Xh = Xh * Mh
    feats, stats, f_peak, peak, total, power = run_hip(ftn, torch.from_numpy(Xh).to(DEV), torch.from_numpy(Mh).to(DEV), True)
    check_against_restatement(Xh, Mh, feats, stats, f_peak, power, "T1913 N512")
    assert ((feats[:, 4] > 6.9) & (feats[:, 4] < 7.1)).sum() > N // 2          # the planted week is found


# ---------------------------------------------------------------- end to end
def test_prepared_table_feeds_device_windows_and_inverse(ftn, fx):
    meta, arrays = fx
    Xh, Mh = arrays["planted:X"], arrays["planted:M"]
    X, M = torch.from_numpy(Xh).to(DEV), torch.from_numpy(Mh).to(DEV)
    (t0, t1), (v0, v1) = ftn.table.holdout_rows(Xh.shape[0], 131)
    sc = ftn.table.SeriesScaler.fit(X[t0:t1], "zscore")
    assert ftn.table._last_backend == "hip"
    statics = ftn.table.series_features(X, M)
    Xn_hip = sc.transform(X)
    assert ftn.table._last_backend == "hip"
    Xn_torch = sc.transform(X, backend="torch")
    mk = lambda tab: ftn.windows.DeviceWindows(tab[v0 - 28:v1], 28, 7, valid_mask=M[v0 - 28:v1], series_static=statics,
                                               series_ids=torch.arange(Xh.shape[1]), batch_size=64, stride=5)
    wa, wb = mk(Xn_hip), mk(Xn_torch)
    assert len(wa) == len(wb) > 1
    for i in range(len(wa)):
        a, b = wa.batch(i), wb.batch(i)
        assert all(torch.equal(p, q) for p, q in zip(a, b))
    # the pipeline layout: a forecast rate [B, H, 1] of batch rows whose series are the batch's ids
    xb, yb, mask, xm, ym, st, ids = wa.batch(1)
    cfg = dict(input_len=28, pred_len=7, d_model=16, d_ff=32, n_layers=2, k_periods=3, kernel_set=[(3, 3), (5, 5)],
               dropout=0.0, activation="gelu", mode="direct", use_checkpoint=False)
    g = torch.Generator().manual_seed(1)
    torch.manual_seed(0)
    model = ftn.models.TimesNet(**cfg).eval().to(DEV)           # the tiny TimesNet of tests/test_gpu_windows.py
    with torch.no_grad():
        model((torch.rand(2, 28, 1, generator=g) + 1.0).to(DEV))
        for p in model.parameters():
            if float(p.abs().sum()) == 0.0:
                p.copy_((0.1 * torch.randn(p.shape, generator=g)).to(DEV))
        rate, dispersion = model(xb)                            # the forward's rate in the table's normalised units
    assert rate.shape == (xb.shape[0], 7, 1) and bool(torch.isfinite(rate).all())
    got = sc.inverse(rate, axis=0, series=ids[:, 0])
    assert ftn.table._last_backend == "hip"
    # the host's inverse_transform + clip on the same rates (io.py:613-614, predict.py:961), in numpy
    pr = sc.pairs()
    r = rate.cpu().numpy()[:, :, 0]
    cols = ids[:, 0].cpu().numpy()
    want = np.zeros_like(r)
    for j, c in enumerate(cols):
        mu, sd = float(pr[c, 0]), float(pr[c, 1])             # Python floats, as the reference's dict holds them
        want[j] = r[j] * sd + mu
    want = np.clip(want, 0.0, None)
    assert torch.equal(got.cpu()[:, :, 0], torch.from_numpy(want))
