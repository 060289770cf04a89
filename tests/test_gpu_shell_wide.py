"""The model shell at 128 < d_model <= 512 on the MI355X (``ftn_*_wide_*``: csrc/shell_wide.hip, the wide part of
csrc/timeproj.hip), form by form, with the metric and bounds of ``test_gpu_shell.py`` / ``test_gpu_timeproj.py``:
``e = |got - ref64| / (sum |x||w| + |other addends|)`` in units of u = 2^-24, asserted ``<= (K + 8) u`` before the
epilogue (a lost piece product of the bf16x3 split shows as about 256 u, so every 16-bit form has a case with
K <= 128 - ``test_every_wide_form_ran`` asserts it), rtol 2e-5 / atol 2e-5 after the embedding's epilogue, rtol 2e-5 /
atol 1e-6 for the heads, and the model tolerance rtol 1e-4 / atol 2e-5 against the CPU mirror.

Measured on the MI355X (the case tables below; ``-s`` prints them; max e of a form and the K it occurred at):
    k_embed_wide_bf<4,4,true> / <8,4,true>    4.1 u / 3.2 u at K = 8 (bound 16 u)
    k_embed_wide_bf<4,4,false> / <8,4,false>  7.6 u / 6.7 u at K = 1 (bound 9 u)
    k_head_wide_bf<2>   4.8 u at K = 256 (bound 264 u), 4.3 u at K = 132 (bound 140 u)
    k_head_wide_bf<1>   3.6 u at K = 260 (bound 268 u)        k_head_wide_f32  5.2 u at K = 260
    k_timeproj_bf       5.9 u at L = 1 (bound 9 u)            k_timeproj_row_wide  2.5 u at L = 5 (bound 13 u)
    model against its fp32 CPU mirror: at most 3.2 % of rtol 1e-4 / atol 2e-5 (d_model 256, direct, context)
"""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from test_gpu_shell import _as_window, _gemm_e, _head_ref, _tail, _window
from test_gpu_timeproj import ATOL, RTOL, _err_u, _operands
from test_shell_wide_host import embed_wide_rule, head_wide_rule, timeproj_wide_rule

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
DS = (132, 192, 256, 260, 512)
SEEN = set()             # kernel names the cases of this module ran
E_TABLE = {}             # form -> [max e, smallest K measured]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a ROCm device"
    return torch.device("cuda:0")


def _record(form, K, e):
    row = E_TABLE.setdefault(form, [0.0, K])
    row[0], row[1] = max(row[0], e), min(row[1], K)
    print(f"{form:24s} K={K:4d}  e = {e:7.2f} u   cap = {K + 8} u")


# ------------------------------------------------------------------------------------------------ value embedding
def _embed_setup(ftn, dev, B, L, N, D, layout, seed):
    g = torch.Generator().manual_seed(seed)
    flat, off, st = _window(B, L, N, layout, g)
    w = torch.randn(D, N, generator=g) / N ** 0.5
    win = _as_window(flat, off, st, B, L, N)
    win_d, w_d = _as_window(flat.to(dev), off, st, B, L, N), w.to(dev)
    form = ftn.runtime.embed_form(win_d, w_d)
    assert form == embed_wide_rule(N, D, st[0] if B > 1 else 0, win_d.data_ptr() & 15, w_d.data_ptr() & 15)
    SEEN.add(form)
    return g, win, w, win_d, w_d, form


EMBED_BL = [(1, 1), (3, 10), (2, 17), (37, 1)]
EMBED_NS = (1, 5, 8, 64, 200)
LAYOUTS = ("plain", "off1", "view", "odd")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("D", DS)
def test_embed_against_fp64(D, layout, ftn, dev):
    """Every N at this (D, layout); (B, L), the add and the LayerNorm rotate so that each appears with every D, N and
    layout somewhere in the table.  The GEMM alone: e <= N + 8; with its epilogue: fp64 at rtol / atol 2e-5."""
    rt = ftn.runtime
    for ni, N in enumerate(EMBED_NS):
        i = ni + 2 * DS.index(D) + 3 * LAYOUTS.index(layout)
        B, L = EMBED_BL[i % 4]
        add_mode, ln_on = [None, "shared", "batch"][(i // 2) % 3], (i // 3) % 2 == 0
        g, win, w, win_d, w_d, form = _embed_setup(ftn, dev, B, L, N, D, layout, seed=1000 + 7 * N + D)
        vec = N % 4 == 0 and layout != "off1" and (layout != "odd" or B == 1)
        assert form == f"k_embed_wide_bf<{4 if D <= 256 else 8},4,{'true' if vec else 'false'}>", (form, N, layout, B)
        got = rt.embed_forward(win_d, w_d, None, None).cpu()
        e, ref = _gemm_e(got, win, w)
        _record(form, N, e)
        assert e <= N + 8, (form, B, L, N, D, e)
        add = None if add_mode is None else torch.randn(B if add_mode == "batch" else 1, L, D, generator=g)
        lnp = ((torch.rand(D, generator=g) + 0.5), torch.randn(D, generator=g), 1e-5) if ln_on else None
        want = ref if add is None else ref + add.double()
        if lnp is not None:
            want = Fn.layer_norm(want, (D,), lnp[0].double(), lnp[1].double(), lnp[2])
        out = rt.embed_forward(win_d, w_d, None if add is None else add.to(dev),
                               None if lnp is None else (lnp[0].to(dev), lnp[1].to(dev), lnp[2]))
        np.testing.assert_allclose(out.cpu().numpy(), want.numpy(), rtol=2e-5, atol=2e-5, err_msg=str((form, B, L, N)))


@pytest.mark.parametrize("N,D,layout", [(64, 132, "plain"), (36, 256, "plain"), (37, 260, "plain"), (64, 512, "off1")])
def test_embed_rows_strided_writes_only_its_rows(N, D, layout, ftn, dev):
    """The rows land in a strided destination between guard values, bit-equal to the one-pass GEMM."""
    rt = ftn.runtime
    B, Lr = 3, 11
    for L in (1, 3):
        g, win, w, win_d, w_d, form = _embed_setup(ftn, dev, B, L, N, D, layout, seed=4000 + N + L)
        want = rt.embed_forward(win_d, w_d, None, None)
        for slot in (0, (Lr - L) // 2, Lr - L):
            out = torch.full((B, Lr, D), -777.25, device=dev)
            rt.embed_rows_strided(win_d, w_d, out, slot)
            assert torch.equal(out[:, slot:slot + L], want), (form, L, slot)
            rest = torch.ones(B, Lr, dtype=torch.bool)
            rest[:, slot:slot + L] = False
            assert bool((out.cpu()[rest] == -777.25).all()), (form, L, slot)


@pytest.mark.parametrize("N,D", [(64, 132), (200, 256), (37, 260), (8, 512)])
def test_embed_row_is_bit_identical_alone_in_a_batch_and_at_the_end_of_300_rows(N, D, ftn, dev):
    rt = ftn.runtime
    g = torch.Generator().manual_seed(N + D)
    x = torch.randn(300, 1, N, generator=g).to(dev)
    w = (torch.randn(D, N, generator=g) / N ** 0.5).to(dev)
    add = torch.randn(1, 1, D, generator=g).to(dev)
    ln = (torch.rand(D, generator=g).to(dev) + 0.5, torch.randn(D, generator=g).to(dev), 1e-5)
    SEEN.add(rt.embed_form(x, w))
    for a, n in ((None, None), (add, ln)):
        full = rt.embed_forward(x, w, a, n)                                  # rows of L = 1: 300 rows, the last tile ragged
        for r in (0, 17, 63, 64, 299):
            assert torch.equal(rt.embed_forward(x[r:r + 1], w, a, n), full[r:r + 1]), r
        assert torch.equal(rt.embed_forward(x[290:], w, a, n), full[290:])
        assert torch.equal(rt.embed_forward(x[3:40], w, a, n), full[3:40])
        as_window = rt.embed_forward(x[4:300].reshape(8, 37, N), w, None if a is None else a.expand(1, 37, D).contiguous(), n)
        assert torch.equal(as_window.reshape(296, 1, D), full[4:300])        # the same rows as 8 windows of 37


def test_embed_row_isolation(ftn, dev):
    """One NaN in x poisons its own output row and nothing else, bit for bit (LayerNorm on: the reductions that cross
    the waves of a workgroup stay inside a row)."""
    rt = ftn.runtime
    B, L, N, D = 3, 23, 64, 260
    g, win, w, win_d, w_d, form = _embed_setup(ftn, dev, B, L, N, D, "plain", seed=5000)
    add = torch.randn(1, L, D, generator=g).to(dev)
    ln = (torch.rand(D, generator=g).to(dev) + 0.5, torch.randn(D, generator=g).to(dev), 1e-5)
    clean = rt.embed_forward(win_d, w_d, add, ln).cpu()
    for b, l, n in [(0, 0, 0), (1, 11, N // 2), (2, L - 1, N - 1)]:
        keep = win_d[b, l, n].clone()
        win_d[b, l, n] = float("nan")
        got = rt.embed_forward(win_d, w_d, add, ln).cpu()
        win_d[b, l, n] = keep
        assert bool(got[b, l].isnan().all()), (form, b, l, n)
        got[b, l] = clean[b, l]
        assert torch.equal(got, clean), (form, b, l, n)


# ------------------------------------------------------------------------------------------------------ ring epilogue
@pytest.mark.parametrize("N", [24, 23], ids=["vec", "generic"])
@pytest.mark.parametrize("D", [132, 256, 512])
@pytest.mark.parametrize("mode", ["none", "shared", "shared_layer", "batch_layer"])
def test_ring_is_bit_equal_to_the_one_pass_embedding(mode, D, N, ftn, dev):
    """Every head slot of an L = 5 ring: against fp64 at the embedding's epilogue tolerance, and bit for bit against
    ``embed_forward`` of the rolled window - the equality that admits the four wide forms to
    ``forecast.RING_EXACT_LAYER_FORMS`` at every d_model, ragged column tiles (132) included."""
    rt = ftn.runtime
    B, L = 5, 5
    g, win, w, win_d, w_d, form = _embed_setup(ftn, dev, B, L, N, D, "plain", seed=6000 + D + N)
    assert form in ftn.forecast.RING_EXACT_LAYER_FORMS
    add = None if mode == "none" else torch.randn(B if mode == "batch_layer" else 1, L, D, generator=g)
    lnp = (torch.rand(D, generator=g) + 0.5, torch.randn(D, generator=g), 1e-5) if mode.endswith("layer") else None
    add_d = None if add is None else add.to(dev)
    ln_d = None if lnp is None else (lnp[0].to(dev), lnp[1].to(dev), lnp[2])
    V = torch.empty(B, L, D, device=dev)
    rt.embed_rows_strided(win_d, w_d, V, 0)
    for head in range(L):
        got = rt.embed_ring(V, head, add_d, ln_d)
        want = torch.roll(V.cpu().double(), -head, dims=1)
        if add is not None:
            want = want + add.double()
        if lnp is not None:
            want = Fn.layer_norm(want, (D,), lnp[0].double(), lnp[1].double(), lnp[2])
        np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), rtol=2e-5, atol=2e-5)
        rolled = torch.roll(win_d, -head, dims=1).contiguous()
        assert torch.equal(got, rt.embed_forward(rolled, w_d, add_d, ln_d)), (form, head)


# ----------------------------------------------------------------------------------------------------- time projection
TP_DS, TP_LS, TP_SS, TP_BS = (132, 192, 260, 512), (1, 5, 33, 96, 336), (1, 2, 17, 96), (1, 3)


@pytest.mark.parametrize("L", TP_LS)
@pytest.mark.parametrize("D", TP_DS)
def test_timeproj_against_fp64(D, L, ftn, dev):
    """Every (S, B) at this (D, L), ``weight[-S:]`` slices on every other case: e <= L + 8."""
    rt = ftn.runtime
    for (si, S), (bi, B) in itertools.product(enumerate(TP_SS), enumerate(TP_BS)):
        sliced = bool((si + bi + TP_DS.index(D) + TP_LS.index(L)) & 1)
        seq, weight, bias = _operands(B, L, S, D, sliced, 1.0, seed=1000 * D + 10 * L + S + B)
        wt, bt = weight[-S:], bias[-S:]
        dw, db, dseq = weight.to(dev)[-S:], bias.to(dev)[-S:], seq.to(dev)
        form = rt.timeproj_form(dseq, dw)
        assert form == timeproj_wide_rule(L, S, D, dw.data_ptr() & 15)
        SEEN.add(form)
        got = rt.timeproj_forward(dseq, dw, db)
        assert got.shape == (B, S, D) and got.is_contiguous()
        e = _err_u(got.cpu(), seq, wt, bt)
        _record(form.split("<")[0], L, e)
        assert e <= L + 8, (form, B, L, S, D, sliced, e)


@pytest.mark.parametrize("S", [1, 17, 100])
@pytest.mark.parametrize("D,L", [(132, 33), (260, 336), (512, 96)])
def test_timeproj_row_is_bit_identical_in_any_batch_and_writes_only_its_output(D, L, S, ftn, dev):
    rt = ftn.runtime
    B = 7
    seq, weight, bias = _operands(B, L, S, D, True, 1.0, seed=D + L + S)
    dseq, dw, db = seq.to(dev), weight.to(dev)[-S:], bias.to(dev)[-S:]
    full = rt.timeproj_forward(dseq, dw, db)
    for b in (0, 3, 6):
        assert torch.equal(rt.timeproj_forward(dseq[b:b + 1], dw, db), full[b:b + 1]), b
    assert torch.equal(rt.timeproj_forward(dseq[2:5], dw, db), full[2:5])
    big = torch.cat([dseq, dseq.flip(0)] * 20)                 # 280 rows
    got = rt.timeproj_forward(big, dw, db)
    assert torch.equal(got[:B], full) and torch.equal(got[-B:], full.flip(0))
    # hidden between guard words in one allocation
    n, pad = B * S * D, 256
    buf = torch.full((pad + n + pad,), 1234.5, device=dev)
    hid = buf[pad:pad + n]
    assert hid.data_ptr() % 16 == 0
    rc = ftn.lib.load().ftn_timeproj_wide_forward(dseq.data_ptr(), B, L, D, dw.data_ptr(), db.data_ptr(), S,
                                                  hid.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    ftn.lib.check(rc, "ftn_timeproj_wide_forward")
    torch.cuda.synchronize()
    assert bool((buf[:pad] == 1234.5).all()) and bool((buf[pad + n:] == 1234.5).all())
    assert torch.equal(hid.view(B, S, D), full)


# -------------------------------------------------------------------------------------------------------------- heads
def _check_heads(ftn, dev, B, S, D, N, hist, layout, late_mode, floor_mode, seed, measure=True, need_loop=False):
    rt = ftn.runtime
    g = torch.Generator().manual_seed(seed)
    hidden = torch.randn(B, S, D, generator=g)
    w_mu, w_sg = 0.3 * torch.randn(N, D, generator=g), 0.3 * torch.randn(N, D, generator=g)
    b_mu, b_sg = torch.randn(N, generator=g), torch.randn(N, generator=g)
    tail, tail_d = _tail(B, hist, N, layout, g, dev)
    tail[0, 0] += 25.0                                # some pre-activations past the softplus threshold
    tail_d[0, 0] += 25.0
    late = None if late_mode is None else 0.5 * torch.randn(B if late_mode == "batch" else 1, S, N, generator=g)
    fv = torch.rand(N, generator=g) if floor_mode == "vector" else None
    to = lambda t: None if t is None else t.to(dev)
    hd, wm, ws = to(hidden), to(w_mu), to(w_sg)
    form, cap = rt.head_form(hd, wm, tail_d, to(late))
    late_bs = S * N if late is not None and late.shape[0] == B and B > 1 else 0
    assert (form, cap) == head_wide_rule(N, D, tail_d.stride(0) if B > 1 else 0, late_bs, tail_d.data_ptr() & 15)
    SEEN.add(form)
    if need_loop:
        assert cap and B * S > 64 * cap and (B * S - 64 * cap) % 16 != 0, (form, cap)   # the row loop iterates, ragged end
    rate, disp, bad = rt.head_forward(hd, wm, to(b_mu), ws, to(b_sg), tail_d, hist, to(late), to(fv), 1e-3)
    want_r, want_d = _head_ref(hidden, w_mu, b_mu, w_sg, b_sg, tail, S, late, fv if fv is not None else 1e-3)
    assert int(bad.item()) == 0
    np.testing.assert_allclose(rate.cpu().numpy(), want_r.numpy(), rtol=2e-5, atol=1e-6)
    np.testing.assert_allclose(disp.cpu().numpy(), want_d.numpy(), rtol=2e-5, atol=1e-6)
    if not measure:
        return form
    # the two GEMMs alone, through elements past the softplus threshold (cf. test_gpu_shell._check_heads): hidden is
    # scaled to get there, tail (zeroed in place: same view, same form), late and the biases are 0
    Sm = max(S, 256 // B + 1)
    hidden = torch.randn(B, Sm, D, generator=g)
    zero_n = torch.zeros(N, device=dev)
    tail_d.zero_()
    assert rt.head_form(to(hidden), wm, tail_d, None)[0] == form
    rate, disp, bad = rt.head_forward(to(hidden) * 30.0, wm, zero_n, ws, zero_n, tail_d, hist, None, None, 1e-3)
    assert int(bad.item()) == 0
    h30 = (hidden * 30.0).reshape(-1, D)
    eps32, floor32 = float(np.float32(1e-6)), float(np.float32(1e-3))
    for name, out, w, extra in (("rate", rate, w_mu, eps32), ("disp", disp, w_sg, floor32 + eps32)):
        ref = h30.double() @ w.double().t()
        den = h30.double().abs() @ w.double().abs().t() + extra
        past = ref > 20.5
        assert int(past.sum()) >= 8, (form, name)
        got = out.cpu().double().reshape(-1, N) - extra
        e = float(((got - ref).abs() / den)[past].max()) / U
        _record(form, D, e)
        assert e <= D + 8, (form, name, e)
    return form


HEAD_NS = (1, 5, 8, 64, 68, 200)
HEAD_BS = [(3, 6, 6), (4, 5, 3), (2, 1, 1)]          # B, S, hist (hist < S: edge-padded)


@pytest.mark.parametrize("N", HEAD_NS)
@pytest.mark.parametrize("D", DS)
def test_heads_against_fp64(D, N, ftn, dev):
    """Every (D, N) on the form its N allows, and every vector N again behind a tail that is one element off or has an
    odd batch stride (the fp32 form); (B, S, hist), late bias and floor rotate through the table."""
    i = DS.index(D) * len(HEAD_NS) + HEAD_NS.index(N)
    B, S, hist = HEAD_BS[i % 3]
    late, floor = [None, "shared", "batch"][(i // 3) % 3], ["scalar", "vector"][i % 2]
    form = _check_heads(ftn, dev, B, S, D, N, hist, "plain", late, floor, seed=7000 + 13 * D + N)
    assert form == (f"k_head_wide_bf<{2 if D <= 256 else 1}>" if N % 4 == 0 else "k_head_wide_f32")
    if N % 4 == 0:
        B, S, hist = HEAD_BS[(i + 1) % 3]
        layout = "off1" if i % 2 or B == 1 else "odd"
        form = _check_heads(ftn, dev, B, S, D, N, hist, layout, [None, "shared", "batch"][(i + 1) % 3],
                            ["scalar", "vector"][(i + 1) % 2], seed=7500 + 13 * D + N)
        assert form == "k_head_wide_f32"


@pytest.mark.parametrize("B,S,D,N", [(3, 5507, 132, 64), (5, 1643, 256, 64), (3, 1371, 512, 64), (7, 4683, 192, 8)])
def test_head_row_loop(B, S, D, N, ftn, dev):
    """Rows beyond 64 x the gridDim.y cap by a non-multiple of 16: a workgroup walks several row tiles and the last
    tile is partial.  Every row is compared."""
    _check_heads(ftn, dev, B, S, D, N, 4, "plain", None, "vector", seed=8000 + D, measure=False, need_loop=True)


@pytest.mark.parametrize("D,N,layout", [(132, 8, "plain"), (256, 64, "plain"), (512, 68, "plain"), (260, 5, "plain"),
                                        (192, 64, "off1")])
def test_head_row_isolation(D, N, layout, ftn, dev):
    """One NaN in ``hidden`` poisons both outputs of its own row only and raises both bits of the flag; every other
    output row keeps its bits."""
    rt = ftn.runtime
    B, S = 3, 23
    g = torch.Generator().manual_seed(9000 + D)
    hidden = torch.randn(B, S, D, generator=g).to(dev)
    w_mu, w_sg = (0.3 * torch.randn(N, D, generator=g)).to(dev), (0.3 * torch.randn(N, D, generator=g)).to(dev)
    b = torch.randn(N, generator=g).to(dev)
    _, tail_d = _tail(B, S, N, layout, g, dev)
    form, _ = rt.head_form(hidden, w_mu, tail_d, None)
    SEEN.add(form)
    r0, d0, bad = rt.head_forward(hidden, w_mu, b, w_sg, b, tail_d, S, None, None, 1e-3)
    assert int(bad.item()) == 0
    r0, d0 = r0.cpu(), d0.cpu()
    for bb, s, k in [(0, 0, 0), (1, 11, D // 2), (2, S - 1, D - 1)]:
        keep = hidden[bb, s, k].clone()
        hidden[bb, s, k] = float("nan")
        r, d, bad = rt.head_forward(hidden, w_mu, b, w_sg, b, tail_d, S, None, None, 1e-3)
        hidden[bb, s, k] = keep
        assert int(bad.item()) == 3, form
        r, d = r.cpu(), d.cpu()
        assert bool(r[bb, s].isnan().all()) and bool(d[bb, s].isnan().all()), (form, bb, s, k)
        r[bb, s], d[bb, s] = r0[bb, s], d0[bb, s]
        assert torch.equal(r, r0) and torch.equal(d, d0), (form, bb, s, k)
    # a row's bits do not depend on the rows that share the call
    r1, d1, _ = rt.head_forward(hidden[1:2].contiguous(), w_mu, b, w_sg, b, tail_d[1:2], S, None, None, 1e-3)
    if layout == "plain":                               # (a one-row batch passes stride 0: the same form only there)
        assert torch.equal(r1.cpu(), r0[1:2]) and torch.equal(d1.cpu(), d0[1:2])


@pytest.mark.parametrize("D,N", [(256, 16), (512, 16), (132, 5)])
def test_head_flag_bits_separately(D, N, ftn, dev):
    """+inf in ``tail`` raises bit 0 only, a NaN in ``b_sigma`` bit 1 only."""
    rt = ftn.runtime
    B, S = 2, 5
    g = torch.Generator().manual_seed(11)
    hidden, w = torch.randn(B, S, D, generator=g).to(dev), (0.1 * torch.randn(N, D, generator=g)).to(dev)
    b, tail = torch.zeros(N, device=dev), torch.randn(B, S, N, generator=g).to(dev)
    bad_tail = tail.clone()
    bad_tail[1, 2, 3] = float("inf")
    assert int(rt.head_forward(hidden, w, b, w, b, bad_tail, S, None, None, 1e-3)[2].item()) == 1
    bad_b = b.clone()
    bad_b[N - 1] = float("nan")
    assert int(rt.head_forward(hidden, w, b, w, bad_b, tail, S, None, None, 1e-3)[2].item()) == 2
    assert int(rt.head_forward(hidden, w, b, w, b, tail, S, None, None, 1e-3)[2].item()) == 0


# -------------------------------------------------------------------------------------------------------- model level
def _mirrors(ftn, dev, mode, d_model, ctx, d_ff=None, n_layers=2, N=24, L=24, H=6, seed=0, norm=None):
    """``test_gpu_timeproj._mirrors`` with the width of the blocks and their number open: the same TimesNet on the CPU
    (torch path) and on the device, lazily built parts woken up, a planted period of 6."""
    cfg = dict(input_len=L, pred_len=H, d_model=d_model, d_ff=d_ff or 2 * d_model, n_layers=n_layers, k_periods=3,
               kernel_set=[(3, 3), (5, 5)], dropout=0.0, activation="gelu", mode=mode, use_checkpoint=False)
    if norm is not None:
        cfg["embed_norm_mode"] = norm
    if ctx:
        cfg.update(id_embed_dim=4, use_zero_mean_context=True, context_rank=4)
    g = torch.Generator().manual_seed(seed + 1)
    kw = {"series_ids": torch.arange(N), "series_static": torch.randn(N, 3, generator=g)} if ctx else {}
    torch.manual_seed(seed)
    cpu = ftn.models.TimesNet(**cfg).eval()
    with torch.no_grad():
        cpu(torch.rand(2, L, N, generator=g) + 1.0, **kw)
        for p in cpu.parameters():                              # wake the zero-initialised heads / context maps
            if float(p.abs().sum()) == 0.0:
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
    gpu = ftn.models.TimesNet(**cfg).eval()
    dkw = {k: v.to(dev) for k, v in kw.items()}
    with torch.no_grad():
        gpu(torch.ones(2, L, N, device=dev), **dkw)
    gpu.load_state_dict(cpu.state_dict(), strict=True)
    t = torch.arange(L, dtype=torch.float32).view(1, L, 1)
    x = torch.rand(5, L, N, generator=g) + 1.5 + torch.sin(2 * torch.pi * t / 6.0)
    return cpu, gpu, x, kw, dkw


MODEL_CASES = [(mode, d, ctx, None, 2) for mode in ("direct", "recursive") for d in (132, 192, 256)
               for ctx in (False, True)] + [("direct", 512, True, 512, 1)]


@pytest.mark.parametrize("mode,d_model,ctx,d_ff,n_layers", MODEL_CASES)
def test_model_forward_matches_its_cpu_mirror(mode, d_model, ctx, d_ff, n_layers, ftn, dev):
    cpu, gpu, x, kw, dkw = _mirrors(ftn, dev, mode, d_model, ctx, d_ff, n_layers)
    with torch.no_grad():
        want_r, want_d = cpu(x, **kw)
    assert cpu._last_embed_backend == "torch" and cpu._last_timeproj_backend == "torch"
    with torch.inference_mode():
        rate, disp = gpu(x.to(dev), **dkw)
    assert (gpu._last_embed_backend, gpu._last_timeproj_backend, gpu._last_head_backend) == ("hip", "hip", "hip")
    assert gpu.period_selector.last_selected_periods.tolist() == cpu.period_selector.last_selected_periods.tolist()
    assert rate.shape == (5, 6 if mode == "direct" else 1, 24)
    err = lambda a, b: float(((a.cpu() - b).abs() / (ATOL + RTOL * b.abs())).max())
    print(f"MODEL_ERR {mode} d_model={d_model} ctx={ctx}: rate {err(rate, want_r):.3f} disp {err(disp, want_d):.3f} of tol")
    np.testing.assert_allclose(rate.cpu().numpy(), want_r.numpy(), rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(disp.cpu().numpy(), want_d.numpy(), rtol=RTOL, atol=ATOL)


def test_graph_replay_is_bit_equal_to_eager(ftn, dev):
    _, gpu, x, _, dkw = _mirrors(ftn, dev, "direct", 192, True)
    x = x.to(dev)
    x2 = x.flip(0) * 1.25
    with torch.inference_mode():
        want = [t.clone() for t in gpu(x, **dkw)]
        want2 = [t.clone() for t in gpu(x2, **dkw)]
    gpu._last_embed_backend = gpu._last_timeproj_backend = gpu._last_head_backend = "unset"
    gf = ftn.graph.GraphedForward(gpu, x, **dkw)
    got = [t.clone() for t in gf(x, **dkw)]
    got2 = [t.clone() for t in gf(x2, **dkw)]
    torch.cuda.synchronize()
    # the capture took the HIP shell: no library GEMM for the embedding, the time projection or the heads
    assert (gpu._last_embed_backend, gpu._last_timeproj_backend, gpu._last_head_backend) == ("hip", "hip", "hip")
    assert all(torch.equal(a, b) for a, b in zip(got, want)) and all(torch.equal(a, b) for a, b in zip(got2, want2))
    assert not torch.equal(want[0], want2[0])


@pytest.mark.parametrize("norm", ["none", "decoupled", "layer"])
def test_recursive_forecasts_are_bit_equal_to_the_loop(norm, ftn, dev, monkeypatch):
    """d_model 192, recursive mode, every norm mode: the device path runs (the ring is used - in "layer" mode because
    the wide forms are in ``RING_EXACT_LAYER_FORMS``) and equals the host loop bit for bit, rates and sample paths."""
    F, rt = ftn.forecast, ftn.runtime
    _, gpu, x, _, dkw = _mirrors(ftn, dev, "recursive", 192, True, norm=norm)
    assert gpu.embedding.embed_norm_mode == norm
    x, H = x.to(dev), 9
    calls = {"ring": 0}
    ring = rt.embed_ring

    def counted(*a, **k):
        calls["ring"] += 1
        return ring(*a, **k)

    monkeypatch.setattr(rt, "embed_ring", counted)
    with torch.inference_mode():
        assert rt.embed_form(x, gpu.embedding.value_embedding.weight) in F.RING_EXACT_LAYER_FORMS
        assert F._device_ok(gpu, x, H, None, None, dkw["series_static"], dkw["series_ids"])
        want_r, want_d = F.forecast_recursive_batch_loop(gpu, x, H, **dkw)
        assert calls["ring"] == 0
        got_r, got_d = F.forecast_recursive_batch(gpu, x, H, **dkw)
        assert calls["ring"] == H                                              # the device path ran
        assert (gpu._last_embed_backend, gpu._last_timeproj_backend, gpu._last_head_backend) == ("hip", "hip", "hip")
        want_s = F.forecast_sample_paths_loop(gpu, x, 5, 3, seed=7, **dkw)
        assert calls["ring"] == H
        got_s = F.forecast_sample_paths(gpu, x, 5, 3, seed=7, **dkw)
        assert calls["ring"] == H + 5
    torch.cuda.synchronize()
    assert got_r.shape == (5, H, 24)
    assert torch.equal(got_r, want_r) and torch.equal(got_d, want_d)
    assert all(torch.equal(a.reshape(b.shape), b) for a, b in zip(got_s, want_s))


# ---------------------------------------------------------------------------------------------------- what ran (last)
def test_every_wide_form_ran():
    """Every wide form was run and compared by the cases above, and every 16-bit form was measured at a K whose bound
    is below the 256 u of a lost piece product: K = N <= 128 for the embedding, K = L <= 128 for the time projection,
    K = D = 132 / 192 for the heads (k_head_wide_bf<1> exists from D = 260 on only: its smallest bound is 268 u, and
    its K loop is the loop of k_head_wide_bf<2>, measured at 140 u)."""
    embed = {f"k_embed_wide_bf<{no},4,{vec}>" for no in (4, 8) for vec in ("true", "false")}
    want = embed | {"k_head_wide_bf<2>", "k_head_wide_bf<1>", "k_head_wide_f32", "k_timeproj_row_wide"} | {
        f"k_timeproj_bf<{n},{w}>" for n in (1, 2, 6) for w in ("true", "false")}
    print("\nform                      min K   max e [u]")
    for form in sorted(E_TABLE):
        e, K = E_TABLE[form]
        print(f"{form:24s} {K:6d} {e:11.2f}")
    assert want <= SEEN, sorted(want - SEEN)
    for form in sorted(embed) + ["k_head_wide_bf<2>", "k_timeproj_bf"]:
        assert form in E_TABLE and E_TABLE[form][1] + 8 < 256, form
    assert E_TABLE["k_head_wide_bf<1>"][1] == 260
