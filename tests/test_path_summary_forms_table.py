"""The dispatch table of the path-summary kernels (``ftn_path_summary_form``; host-only, no GPU needed): the reported
form equals the rule restated in tests/paths_checks.py for every shape the GPU test uses, at the boundaries of P and
for strides and addresses that break alignment; and ``ftn_path_summary`` turns bad arguments down on the host, before
any launch."""
import ctypes as C

import pytest

import paths_checks as pc


def _raw(ftn, P, N, window=1, ps=0, bs=0, ybs=0, mis=0):
    return ftn.lib.load().ftn_path_summary_form(P, N, window, ps, bs, ybs, mis)


@pytest.mark.parametrize("P", pc.PATHS + [4, 8, 9, 32, 33, 129, 256, 512, 513])
def test_form_of_every_tested_shape(P, ftn):
    rt = ftn.runtime
    for B, H, N in pc.SHAPES:
        row = H * N
        quad = N % 4 == 0
        dense = (B * row if P > 1 else 0, row if B > 1 else 0, row if B > 1 else 0)
        for window in (1, 2 if H % 2 == 0 else 1, H):
            assert rt.path_summary_form_of(P, N, window, dense, 0) == pc.form(P, quad), (P, B, H, N)
        for mis in (4, 8, 12):                                  # a misaligned base address
            assert rt.path_summary_form_of(P, N, 1, dense, mis) == pc.form(P, False)
        if B > 1:                                               # a stride that breaks, and one that keeps, the quads
            assert rt.path_summary_form_of(P, N, 1, (dense[0] + 2 * B, row + 2, row), 0) == pc.form(P, False)
            assert rt.path_summary_form_of(P, N, 1, (dense[0], row, row + 2), 0) == pc.form(P, False)
            assert rt.path_summary_form_of(P, N, 1, (dense[0] + 4 * B, row + 4, row + 8), 0) == pc.form(P, quad)
        if P > 1:
            assert rt.path_summary_form_of(P, N, 1, (dense[0] + 3, dense[1], dense[2]), 0) == pc.form(P, False)
            assert rt.path_summary_form_of(P, N, 1, (dense[0] + 64, dense[1], dense[2]), 0) == pc.form(P, quad)


def test_form_word_fields(ftn):
    L = ftn.lib
    assert L.FTN_PATHS_MAX == 1024 and (L.FTN_PATH_SUM, L.FTN_PATH_MAX, L.FTN_PATH_LDS) == (0, 1, 16)
    assert {"ftn_path_summary", "ftn_path_summary_form"} <= set(L.EXPORTS)
    for P, pp, T in ((1, 2, 0), (2, 2, 0), (3, 4, 0), (16, 16, 0), (17, 32, 0), (64, 64, 0), (65, 128, 64),
                     (128, 128, 64), (129, 256, 64), (256, 256, 64), (257, 512, 32), (512, 512, 32), (513, 1024, 16),
                     (1024, 1024, 16)):
        f = _raw(ftn, P, 8)
        assert (f >> 8) & 0xFFF == pp and f >> 20 == T and bool(f & L.FTN_PATH_LDS) == (pp > 64), P
        assert bool(f & 2) == (pp <= 16 or pp > 64) and not _raw(ftn, P, 7) & 2 and not _raw(ftn, P, 8, mis=4) & 2
        assert pp * T * 4 <= 65536


def test_form_rejects_bad_arguments(ftn):
    lib = ftn.lib.load()
    assert _raw(ftn, 0, 8) < 0 and _raw(ftn, 1025, 8) < 0 and _raw(ftn, 4, 0) < 0 and _raw(ftn, 4, 8, window=0) < 0
    assert _raw(ftn, 4, 8, ps=-1) < 0 and _raw(ftn, 4, 8, bs=-4) < 0 and _raw(ftn, 4, 8, ybs=-4) < 0
    assert _raw(ftn, 4, 8, mis=2) < 0 and _raw(ftn, 4, 8, mis=16) < 0 and _raw(ftn, 4, 8, mis=-4) < 0
    assert b"ftn_path_summary_form" in lib.ftn_last_error()
    with pytest.raises(ValueError, match="ftn_path_summary_form"):
        ftn.runtime.path_summary_form_of(2000, 8)


def test_entry_rejects_bad_arguments_before_any_launch(ftn):
    """Every call below fails a host check; the pointers are never dereferenced and nothing is enqueued, so the
    addresses need not be device memory."""
    lib = ftn.lib.load()
    X, Y, O = 0x10000, 0x20000, 0x30000

    def call(x=X, ps=48, bs=24, P=4, B=2, H=3, N=8, window=1, reduce=0, y=Y, ybs=24, ranks=(1, 4), Q=None, q=O,
             mean=O + 0x1000, crps=O + 0x2000, srt=None):
        arr = (C.c_int * max(len(ranks), 1))(*ranks)
        return lib.ftn_path_summary(x, ps, bs, P, B, H, N, window, reduce, y, ybs, arr if ranks else None,
                                    len(ranks) if Q is None else Q, q, mean, crps, srt, None)

    assert call(x=None) < 0
    assert call(P=0) < 0 and call(P=1025) < 0 and call(B=0) < 0 and call(H=0) < 0 and call(N=0) < 0
    assert call(window=2) < 0 and call(window=0) < 0 and call(reduce=2) < 0 and call(reduce=-1) < 0
    assert call(ranks=(0,)) < 0 and call(ranks=(5,)) < 0 and call(ranks=(1, 2, 3, 4, 1, 2, 3, 4, 1)) < 0
    assert call(Q=-1) < 0 and call(q=None) < 0 and call(ranks=(), Q=2) < 0
    assert call(y=None) < 0                                     # crps_out without y
    assert call(ranks=(), q=None, mean=None, crps=None) < 0     # nothing to compute
    assert call(bs=23) < 0 and call(ybs=8) < 0 and call(ps=47) < 0 and call(ps=-48) < 0
    assert call(x=X + 2) < 0 and call(mean=O + 0x1001) < 0
    assert call(B=1 << 20, H=1 << 10, N=1 << 10, bs=1 << 20, ps=1 << 40, ybs=1 << 20) < 0     # B H' N beyond int32
    assert b"ftn_path_summary" in lib.ftn_last_error()
