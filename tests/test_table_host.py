"""Table preparation without a GPU: the torch backend of ``table`` against everything the reference returned on the
fixture tables (tests/golden/table_cases.npz) - features, scaler pairs, the normalised train rows, the transformed
validation rows, the inverse with its clip, and the row ranges of the two split functions - and every argument check of
``ftn_table_moments``, ``ftn_table_spectrum`` and ``ftn_table_affine`` through the C ABI, which the host makes before
any launch.

The torch backend's reductions run in numpy on the tensors' memory, the reference's own expressions in the reference's
own order, so every comparison here is for equal bits: no reduction order of torch enters and no tolerance is needed."""
import ctypes as C

import numpy as np
import pytest
import torch

import table_checks as tc


@pytest.fixture(scope="module")
def fx():
    return tc.fixture()


def test_exports_and_abi(ftn):
    L = ftn.lib
    names = {"ftn_table_moments", "ftn_table_moments_bytes", "ftn_table_moments_form", "ftn_table_spectrum",
             "ftn_table_spectrum_bytes", "ftn_table_spectrum_form", "ftn_table_twiddle_bytes", "ftn_table_twiddle_init",
             "ftn_table_features", "ftn_table_scaler", "ftn_table_affine", "ftn_table_affine_form"}
    assert names <= set(L.EXPORTS)
    assert L.ABI_VERSION == 14 and L.load().ftn_abi_version() == 14
    assert (L.FTN_TAB_SPEC_COLS, L.FTN_TAB_SPEC_BINS, L.FTN_TAB_SPEC_CHUNK, L.FTN_TAB_PARTIALS_MAX) == (
        tc.COLS, tc.BINS, tc.CHUNK, tc.PARTIALS_MAX)
    assert ftn.table.FEATURE_NAMES == tc.FEATURES
    assert L.load().ftn_table_twiddle_bytes(731) == 731 * 8 and L.load().ftn_table_twiddle_bytes(65537) == 0
    assert L.load().ftn_table_spectrum_bytes(65537, 4) == 0 and L.load().ftn_table_spectrum_bytes(731, 37) == 3 * 37 * 16
    assert L.load().ftn_table_moments_bytes(731, 37) == 23 * 10 * 37 * 8


@pytest.mark.parametrize("name", ["planted", "mixed", "neg", "t1", "t2", "t3"])
def test_torch_features_are_the_reference(name, ftn, fx):
    meta, arrays = fx
    X, M = torch.from_numpy(arrays[f"{name}:X"]), torch.from_numpy(arrays[f"{name}:M"])
    got = ftn.table.series_features(X, M)
    assert ftn.table._last_backend == "torch" and got.dtype == torch.float32 and got.shape == (X.shape[1], 5)
    assert tc.same_bits(got, torch.from_numpy(arrays[f"{name}:features"]))
    # slices of a larger table are read in place and give the same bits
    big = torch.full((X.shape[0] + 3, X.shape[1] + 5), float("nan"))
    bigm = torch.zeros_like(big)
    big[2:-1, 4:-1], bigm[2:-1, 4:-1] = X, M
    assert tc.same_bits(ftn.table.series_features(big[2:-1, 4:-1], bigm[2:-1, 4:-1]), got)


@pytest.mark.parametrize("name", ["planted", "mixed", "neg", "t1", "t2", "t3"])
def test_torch_scaler_is_the_reference(name, ftn, fx):
    meta, arrays = fx
    m = meta["tables"][name]
    X = torch.from_numpy(arrays[f"{name}:X"])
    (a0, a1), (v0, v1) = m["train"], m["val"]
    pred = torch.from_numpy(arrays[f"{name}:pred"])
    for method, per_series in tc.FITS:
        key = tc.fit_key(name, method, per_series)
        sc = ftn.table.SeriesScaler.fit(X[a0:a1], method, per_series=per_series, clip_negative=m["clip"])
        assert ftn.table._last_backend == "torch" and sc.loc.dtype == torch.float32 and sc.n_series == X.shape[1]
        assert np.array_equal(sc.pairs(), arrays[f"{key}:pairs"]), key
        if m["xn"]:                                             # the fit's own normalised rows (the eps rule)
            assert torch.equal(sc.transform(X[a0:a1], clip_negative=m["clip"]), torch.from_numpy(arrays[f"{key}:Xn"])), key
        # a loaded scaler follows _transform_dataframe and inverse_transform (their != 0 rule)
        ld = ftn.table.SeriesScaler.from_pairs(method, arrays[f"{key}:pairs"], device="cpu")
        assert np.array_equal(ld.pairs(), arrays[f"{key}:pairs"])
        if f"{key}:val" not in arrays:                          # the large table's global fits: pairs only
            assert name == "planted" and not per_series
            continue
        assert torch.equal(ld.transform(X[v0:v1], clip_negative=m["clip"]), torch.from_numpy(arrays[f"{key}:val"])), key
        assert torch.equal(ld.inverse(pred), torch.from_numpy(arrays[f"{key}:inv"])), key
        buf = X[v0:v1].clone()
        assert ld.transform(buf, out=buf, clip_negative=m["clip"]) is buf
        assert torch.equal(buf, torch.from_numpy(arrays[f"{key}:val"]))


def test_from_pairs_takes_the_reference_dict(ftn):
    sc = ftn.table.SeriesScaler.from_pairs("minmax", {"b": (1.0, 3.0), "a": (2.0, 2.0)}, ids=["a", "b"], device="cpu")
    assert sc.loc.tolist() == [2.0, 1.0] and sc.scale.tolist() == [1.0, 2.0] and sc.pairs().tolist() == [[2, 2], [1, 3]]
    z = ftn.table.SeriesScaler.from_pairs("zscore", [[5.0, 0.0], [1.0, 2.0]], device="cpu")
    assert z.scale.tolist() == [1.0, 2.0] and z.inv_scale.tolist() == [0.0, 2.0]          # train.py:584, io.py:614
    with pytest.raises(ValueError, match="method"):
        ftn.table.SeriesScaler.from_pairs("none", [[0.0, 1.0]])
    with pytest.raises(ValueError, match=r"\[N, 2\]"):
        ftn.table.SeriesScaler.from_pairs("zscore", [1.0, 2.0, 3.0])


def test_inverse_axis_and_series_map(ftn):
    """The pipeline layout: a series is a batch row, ``series`` maps rows to table columns (repeated, out of order)."""
    g = np.random.default_rng(5)
    pairs = np.stack([g.uniform(-3, 3, 7), g.uniform(0.5, 4, 7)], axis=1)
    sc = ftn.table.SeriesScaler.from_pairs("zscore", pairs, device="cpu")
    ids = torch.tensor([6, 0, 0, 3, 5, 1])
    pred = torch.from_numpy(g.standard_normal((2, 6, 4, 1)).astype(np.float32))
    got = sc.inverse(pred, axis=1, series=ids)
    want = pred * sc.scale[ids].view(1, 6, 1, 1)
    want = torch.clamp(want + sc.loc[ids].view(1, 6, 1, 1), min=0)
    assert torch.equal(got, want)
    assert torch.equal(sc.inverse(pred, axis=1, series=ids, clip=False).clamp(min=0), want)
    wide = torch.from_numpy(g.standard_normal((3, 4, 7)).astype(np.float32))
    assert torch.equal(sc.inverse(wide), torch.clamp(wide * sc.scale + sc.loc, min=0))
    with pytest.raises(ValueError, match="series"):
        sc.inverse(pred, axis=1)
    with pytest.raises(ValueError, match="series must map"):
        sc.inverse(pred, axis=1, series=ids[:-1])
    for bad in ([6, 0, 0, 3, 7, 1], torch.tensor([6, 0, -1, 3, 5, 1])):                # host maps are validated
        with pytest.raises(ValueError, match=r"outside 0\.\.6"):
            sc.inverse(pred, axis=1, series=bad)
    ftn.table._last_backend = None
    none = ftn.table.SeriesScaler.fit(wide[0], "none")
    assert ftn.table._last_backend is None                      # nothing ran
    assert torch.equal(none.transform(wide[0]), wide[0]) and none.pairs() is None


def test_row_ranges(ftn, fx):
    meta, _ = fx
    assert len(meta["splits"]) == 27
    for s in meta["splits"]:
        if s["kind"] == "holdout":
            got = [ftn.table.holdout_rows(s["T"], *s["args"])]
        else:
            got = ftn.table.rolling_rows(s["T"], *s["args"])
        assert [[list(a), list(b)] for a, b in got] == s["ranges"], s
    with pytest.raises(ValueError, match="positive"):
        ftn.table.holdout_rows(10, 0)


def test_backend_choice(ftn):
    X = torch.zeros(4, 3)
    with pytest.raises(ValueError, match="ROCm"):
        ftn.table.series_features(X, backend="hip")
    with pytest.raises(ValueError, match="backend"):
        ftn.table.series_features(X, backend="numpy")
    with pytest.raises(ValueError, match="same shape"):
        ftn.table.series_features(X, torch.ones(4, 2))
    with pytest.raises(ValueError, match="method"):
        ftn.table.SeriesScaler.fit(X, "robust")


# ---------------------------------------------------------------- the C ABI rejects before any launch
A = 0x7f0000000000                                              # stand-in device addresses: no call below reaches a launch


def _rejected(ftn, rc, text):
    msg = ftn.lib.load().ftn_last_error().decode()
    assert rc == -1 and text in msg, (rc, msg)


def test_moments_argument_checks(ftn):
    L, lib = ftn.lib, ftn.lib.load()

    def args(**kw):
        a = L.FtnTableMomentsArgs()
        a.X, a.x_stride, a.M, a.m_stride, a.T, a.N, a.flags = A, 8, A + 4096, 8, 10, 8, L.FTN_TAB_MASK
        a.stats, a.workspace, a.workspace_bytes = A + 8192, A + 16384, lib.ftn_table_moments_bytes(10, 8)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    cases = [(dict(T=0), "must be positive"), (dict(N=0), "must be positive"), (dict(flags=8), "flags=8"),
             (dict(X=None), "null X"), (dict(x_stride=7), "X row stride 7"), (dict(M=None), "FTN_TAB_MASK without M"),
             (dict(m_stride=5), "M row stride 5"), (dict(X=A + 2), "4-byte aligned"),
             (dict(T=1 << 60), "pass 64 bits"), (dict(stats=None), "stats must be"), (dict(stats=A + 4), "stats must be"),
             (dict(workspace=None), "workspace"), (dict(workspace_bytes=8), "workspace holds 8 bytes")]
    for kw, text in cases:
        _rejected(ftn, lib.ftn_table_moments(C.byref(args(**kw)), None), text)
    _rejected(ftn, lib.ftn_table_moments(None, None), "null arguments")
    f = L.FtnTableForm()
    _rejected(ftn, lib.ftn_table_moments_form(C.byref(args(N=-1)), C.byref(f)), "must be positive")
    _rejected(ftn, lib.ftn_table_moments_form(C.byref(args()), None), "null form")
    assert lib.ftn_table_moments_form(C.byref(args()), C.byref(f)) == 0 and f.load_bytes == 16
    assert lib.ftn_table_moments_bytes(0, 8) == 0 and lib.ftn_table_moments_bytes(8, 0) == 0


def test_spectrum_argument_checks(ftn):
    L, lib = ftn.lib, ftn.lib.load()

    def args(**kw):
        a = L.FtnTableSpectrumArgs()
        a.X, a.x_stride, a.M, a.m_stride, a.T, a.N = A, 8, A + 4096, 8, 10, 8
        a.mean, a.twiddle, a.f_peak, a.peak, a.total = A + 8192, A + 12288, A + 16384, A + 20480, A + 24576
        a.workspace, a.workspace_bytes = A + 32768, lib.ftn_table_spectrum_bytes(10, 8)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    cases = [(dict(T=0), "outside the supported 1..65536"), (dict(T=65537), "outside the supported 1..65536"),
             (dict(T=1 << 40), "outside the supported"), (dict(N=0), "N=0"), (dict(X=None), "null X"),
             (dict(x_stride=7), "X row stride 7"), (dict(m_stride=7), "M row stride 7"), (dict(M=A + 1), "4-byte aligned"),
             (dict(x_stride=1 << 60), "pass 64 bits"), (dict(mean=None), "null mean or twiddle"),
             (dict(twiddle=None), "null mean or twiddle"), (dict(twiddle=A + 4), "8-byte aligned"),
             (dict(f_peak=None), "null output"), (dict(peak=None), "null output"), (dict(total=None), "null output"),
             (dict(power_out=A + 2), "outputs must be 4-byte aligned"), (dict(workspace=None), "workspace"),
             (dict(workspace_bytes=0), "workspace holds 0 bytes")]
    for kw, text in cases:
        _rejected(ftn, lib.ftn_table_spectrum(C.byref(args(**kw)), None), text)
    _rejected(ftn, lib.ftn_table_spectrum(None, None), "null arguments")
    _rejected(ftn, lib.ftn_table_twiddle_init(A, 65537, None), "outside 1..65536")
    _rejected(ftn, lib.ftn_table_twiddle_init(None, 8, None), "8-byte aligned")
    f = L.FtnTableForm()
    _rejected(ftn, lib.ftn_table_spectrum_form(C.byref(args(T=65537)), C.byref(f)), "outside the supported")
    _rejected(ftn, lib.ftn_table_features(A, A, A, A, 0, 4, A, None), "must be positive")
    _rejected(ftn, lib.ftn_table_features(A, A, None, A, 5, 4, A, None), "null pointer")
    _rejected(ftn, lib.ftn_table_features(A + 4, A, A, A, 5, 4, A, None), "8-byte")
    _rejected(ftn, lib.ftn_table_scaler(A, 0, 0, 1, 1e-8, A, A, A, None), "N=0")
    _rejected(ftn, lib.ftn_table_scaler(A, 4, 2, 1, 1e-8, A, A, A, None), "method=2")
    _rejected(ftn, lib.ftn_table_scaler(A, 4, 0, 1, float("nan"), A, A, A, None), "eps is NaN")
    _rejected(ftn, lib.ftn_table_scaler(A, 4, 0, 1, 1e-8, A, None, A, None), "null pointer")


def test_affine_argument_checks(ftn):
    L, lib = ftn.lib, ftn.lib.load()

    def args(**kw):
        a = L.FtnTableAffineArgs()
        a.x, a.out, a.loc, a.scale = A, A + 65536, A + 4096, A + 8192
        a.outer, a.S, a.inner, a.n_cols = 3, 8, 4, 8
        a.x_ostride, a.x_sstride, a.o_ostride, a.o_sstride = 32, 4, 32, 4
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    cases = [(dict(outer=0), "must be positive"), (dict(S=0), "must be positive"), (dict(inner=0), "must be positive"),
             (dict(S=1 << 20, inner=1 << 11, n_cols=1 << 20), "is not below 2^31"), (dict(flags=2), "flags=2"),
             (dict(n_cols=0), "do not fit"), (dict(n_cols=7), "do not fit the 7 columns"),
             (dict(x_sstride=3), "series strides"), (dict(o_sstride=3), "series strides"),
             (dict(o_ostride=31), "output rows would overlap"), (dict(x_ostride=-1), "output rows would overlap"),
             (dict(x=None), "null pointer"), (dict(out=None), "null pointer"), (dict(loc=None), "null pointer"),
             (dict(scale=None), "null pointer"), (dict(x=A + 2), "4-byte"), (dict(series=A + 4), "8-byte aligned"),
             (dict(x_ostride=1 << 61), "pass 64 bits")]
    for kw, text in cases:
        _rejected(ftn, lib.ftn_table_affine(C.byref(args(**kw)), None), text)
    _rejected(ftn, lib.ftn_table_affine(None, None), "null arguments")
    f = L.FtnTableForm()
    _rejected(ftn, lib.ftn_table_affine_form(C.byref(args(S=0)), C.byref(f)), "must be positive")
    assert lib.ftn_table_affine_form(C.byref(args(n_cols=7, series=A + 8)), C.byref(f)) == 0 and f.lane_axis == 1
