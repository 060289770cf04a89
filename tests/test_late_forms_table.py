"""The dispatch of the late-bias refit, pinned without a GPU: ``ftn_late_backward_form`` and
``ftn_late_backward_workspace`` over the shape grid of tests/late_fit_oracle.py and at the chunk rule's edges, the
workspace of ``ftn_refit_update_list``, and the argument errors of the four launch entries, every one raised before
anything is enqueued (the addresses here are stand-ins nothing may touch)."""
import ctypes as C

import pytest

import late_fit_oracle as oracle

CHUNK = oracle.CHUNK


def _need(R, ctx, S, chunks):
    return 4 * (R * (2 * S + 3 * ctx) + chunks * (S * (ctx + 1) + S + 2 * ctx))


@pytest.mark.parametrize("i", range(len(oracle.GRID)))
def test_form_and_workspace_over_the_grid(i, ftn):
    rt = ftn.runtime
    ctx, S, R, layout = oracle.GRID[i]
    B, Bc, N = oracle.dims(R, layout)
    assert Bc * N == R and Bc in (1, B)
    chunks = -(-R // CHUNK)
    assert rt.late_backward_form_of(B, Bc, N, ctx, S) == ("k_late_bwd_mfma", chunks)
    assert rt.late_backward_workspace(B, Bc, N, ctx, S) == _need(R, ctx, S, chunks)


def test_the_chunk_grows_beyond_256_chunks(ftn):
    rt, L = ftn.runtime, ftn.lib
    assert (L.FTN_LATEFIT_MFMA, L.FTN_LATEFIT_CHUNKS_MAX, L.LATEFIT_CHUNK) == (1, 256, CHUNK)
    cap = L.FTN_LATEFIT_CHUNKS_MAX
    assert rt.late_backward_form_of(1, 1, CHUNK * cap, 64, 96) == ("k_late_bwd_mfma", cap)
    # one row more: ceil(R / 256) = 257 rows a chunk, made even: 258
    R = CHUNK * cap + 1
    assert rt.late_backward_form_of(2, 1, R, 64, 96) == ("k_late_bwd_mfma", -(-R // 258))
    assert rt.late_backward_form_of(R, R, 1, 3, 1) == ("k_late_bwd_mfma", -(-R // 258))
    R = 1 << 20
    assert rt.late_backward_form_of(1, 1, R, 8, 4) == ("k_late_bwd_mfma", cap)
    assert rt.late_backward_workspace(1, 1, R, 8, 4) == _need(R, 8, 4, cap)
    # the pipeline shape and the bench shape of tools/late_fit_time.py
    assert rt.late_backward_form_of(4096, 4096, 1, 64, 96) == ("k_late_bwd_mfma", 16)
    assert rt.late_backward_form_of(32, 1, 512, 64, 96) == ("k_late_bwd_mfma", 2)


def test_shapes_the_backward_does_not_take(ftn):
    rt = ftn.runtime
    for B, Bc, N, ctx, S in ((4, 2, 8, 16, 4), (0, 1, 8, 16, 4), (4, 4, 0, 16, 4), (4, 4, 8, 0, 4), (4, 4, 8, 257, 4),
                             (4, 4, 8, 16, 0), (1, 3, 8, 16, 4)):
        with pytest.raises(ValueError, match="ftn_late_backward_form: B="):
            rt.late_backward_form_of(B, Bc, N, ctx, S)
        assert rt.late_backward_workspace(B, Bc, N, ctx, S) == 0


def test_launch_entries_refuse_bad_arguments_before_any_launch(ftn):
    lib, L = ftn.lib.load(), ftn.lib
    A = [0x10000 * (k + 1) for k in range(16)]                   # stand-in addresses on the 16-byte grid

    def fwd(rows=A[0], n_items=8, lst=None, Bc=2, N=4, ctx=16, S=4, g=A[1], b=A[2], eps=1e-5, w=A[3], bb=A[4],
            gate=A[5], late=A[6]):
        return lib.ftn_late_fit_forward(rows, n_items, lst, Bc, N, ctx, S, g, b, eps, w, bb, gate, late, None)

    def bwd(dpre=A[7], B=2, rows=A[0], n_items=8, lst=None, Bc=2, N=4, ctx=16, S=4, g=A[1], gate=A[5], dw=A[10],
            ws=A[13], ws_bytes=1 << 20):
        return lib.ftn_late_backward(dpre, B, rows, n_items, lst, Bc, N, ctx, S, g, A[2], 1e-5, A[3], A[4], gate, A[8],
                                     A[9], dw, A[11], A[12], ws, ws_bytes, None)

    def refused(rc, name, match):
        with pytest.raises(ValueError, match=match):
            L.check(rc, name)

    f, b = "ftn_late_fit_forward", "ftn_late_backward"
    refused(fwd(rows=None), f, "null pointer")
    refused(fwd(gate=None), f, "null pointer")
    refused(fwd(late=None), f, "late is null")
    refused(fwd(ctx=257), f, r"ctx=257 \(1\.\.256\)")
    refused(fwd(ctx=0), f, r"ctx=0 \(1\.\.256\)")
    refused(fwd(S=0), f, "S=0")
    refused(fwd(Bc=0), f, "Bc=0")
    refused(fwd(w=A[3] + 2), f, "4-byte aligned")
    refused(fwd(lst=A[14] + 4), f, "row list must be 8-byte aligned")
    refused(fwd(lst=A[14], n_items=0), f, "n_items=0")
    refused(fwd(eps=float("nan")), f, "eps is NaN")
    refused(bwd(dpre=None), b, "null pointer")
    refused(bwd(ws=None), b, "null pointer")
    refused(bwd(B=3), b, "Bc must be 1 or B")
    refused(bwd(ctx=300), b, r"ctx=300 \(1\.\.256\)")
    refused(bwd(dw=A[10] + 1), b, "4-byte aligned")
    refused(bwd(lst=A[14], n_items=-1), b, "n_items=-1")
    need = _need(8, 16, 4, 1)
    refused(bwd(ws_bytes=need - 1), b, f"workspace of {need - 1} bytes, {need} needed")


def test_runtime_wrappers_refuse_host_tensors(ftn):
    """The Python entries check their operands themselves: CPU tensors never reach the library."""
    import torch

    rt = ftn.runtime
    rows, params, d_pre = oracle.case(1)
    with pytest.raises(ValueError, match="late_fit_forward: series rows must be a contiguous fp32 device tensor"):
        rt.late_fit_forward(rows, *params, oracle.EPS)
    with pytest.raises(ValueError, match="late_backward: series rows must be"):
        rt.late_backward(d_pre, rows, *params, oracle.EPS)
    with pytest.raises(ValueError, match="late_fit_forward takes an item store"):
        rt.late_fit_forward(rows, *params, oracle.EPS, rows=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"refit_update_list: 33 tensors \(1\.\.32 per call\)"):
        rt.refit_update_list(*([[torch.zeros(1)] * 33] * 4), torch.zeros(1), torch.zeros(2, dtype=torch.int32))


def test_refit_update_list_workspace_and_errors(ftn):
    lib, L = ftn.lib.load(), ftn.lib
    assert L.FTN_REFIT_LIST_MAX == 4

    def ws(*records):
        n = len(records)
        nts = (C.c_int * max(n, 1))(*(len(r) for r in records))
        arrs = [(C.c_longlong * max(len(r), 1))(*r) for r in records]
        ptrs = (C.POINTER(C.c_longlong) * max(n, 1))(*(C.cast(a, C.POINTER(C.c_longlong)) for a in arrs))
        return lib.ftn_refit_update_list_workspace(n, nts, ptrs)

    one = (4097, 1, 3, 4, 5, 7, 64, 193)
    single = lib.ftn_refit_update_workspace(8, (C.c_longlong * 8)(*one))
    assert ws(one) == single
    # records are cut into chunks each on its own: 1025 + 1 + 1 + 1 + 2 + 2 + 16 + 49 = 1097 units -> 2 chunks; then
    # 1025 + 64 + 256 = 1345 units -> 2 chunks
    assert ws(one, (4097, 255, 1023)) == 8 * (2 + 2) + 16
    assert ws((4,), (4,), (4,), (4,)) == 8 * 4 + 16
    assert ws() == 0 and ws((4,), (4,), (4,), (4,), (4,)) == 0 and ws((4,), (0,)) == 0 and ws((4,) * 9) == 0

    def args(counts=(8, 8)):
        a = L.FtnRefitArgs()
        for i, n in enumerate(counts):
            a.p[i], a.g[i], a.m[i], a.v[i] = (0x10000 * (4 * i + k + 1) for k in range(4))
            a.n[i] = n
        a.n_tensors = len(counts)
        a.beta1, a.beta2, a.eps = 0.9, 0.999, 1e-8
        a.lr, a.state = 0x900000, 0x900100
        return a

    def refused(recs, match, ws_ptr=0xA00000, ws_bytes=1 << 16):
        arr = (L.FtnRefitArgs * max(len(recs), 1))(*recs)
        with pytest.raises(ValueError, match=match):
            L.check(lib.ftn_refit_update_list(arr, len(recs), ws_ptr, ws_bytes, None), "ftn_refit_update_list")

    refused([], r"0 records \(1\.\.4\)")
    refused([args()] * 5, r"5 records \(1\.\.4\)")
    refused([args(), args(counts=(8, 0))], "ftn_refit_update_list: tensor 1 has 0 elements")
    other = args()
    other.beta1 = 0.8
    refused([args(), other], "record 1 differs from record 0")
    other = args()
    other.lr = 0x900200
    refused([args(), other], "record 1 differs from record 0")
    refused([args(), args()], "workspace of 8 bytes, 32 needed", ws_bytes=8)
    refused([args(), args()], "on the 8-byte grid", ws_ptr=0xA00004)
    # one record: ftn_refit_update's own checks (the grid form needs the workspace)
    refused([args(counts=(20000, 8))], "ftn_refit_update: workspace of 8 bytes, 56 needed", ws_bytes=8)
