"""The model-shell kernels of ``csrc/shell.hip`` (value embedding, ring epilogue, rate / dispersion heads) and
``k_resid_ln`` on the MI355X, form by form: every case asserts which kernel the library reports
(``runtime.embed_form`` / ``runtime.head_form``, the function the launch dispatches through) and compares with the
operation restated in plain fp64 torch on the CPU.  Inputs are drawn in fp32 and promoted, so both sides see the same
numbers.

Error measure of the two GEMMs, taken before the epilogue: for every output element
``e = |got - ref64| / (sum_k |x_k| |w_k| + |every other addend|)`` in units of ``u = 2^-24``, asserted
``<= (K + 8) u`` - the a-priori bound of any fp32 accumulation of K terms plus the 2^-24-order terms the three-piece
split drops and the output rounding (derived, not measured).  A lost piece product of the bf16x3 split shows as about
256 u, so every 16-bit form has cases with K <= 128.  The same ``e`` of torch's fp32 ``F.linear`` on the CPU is recorded
beside it; ``test_every_form_ran`` prints the table (``-s``).  After the epilogue the tolerances are those of
``test_gpu_parity.py``: rtol 2e-5 / atol 2e-5 (embedding), rtol 2e-5 / atol 1e-6 (heads).

The environment switches FTN_EMBED_F32 / FTN_EMBED_RT / FTN_HEAD_F32 move the cases onto the other forms; the expected
form follows them (``test_gpu_switches.py`` runs this file under each)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from test_shell_forms_table import embed_rule, head_rule

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
SW_E = {"f32": int(os.getenv("FTN_EMBED_F32", "0") or 0) != 0, "rt": int(os.getenv("FTN_EMBED_RT", "0") or 0)}
SW_H = {"f32": int(os.getenv("FTN_HEAD_F32", "0") or 0) != 0}
DEFAULT_ENV = not (SW_E["f32"] or SW_E["rt"] or SW_H["f32"])
SEEN = set()             # kernel names the cases of this module ran
E_TABLE = {}             # form -> [max e of the kernel, max e of torch's fp32 F.linear on the CPU, smallest K]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a ROCm device"
    return torch.device("cuda:0")


def _record(form, K, e_kernel, e_ref):
    row = E_TABLE.setdefault(form, [0.0, 0.0, K])
    row[0], row[1], row[2] = max(row[0], e_kernel), max(row[1], e_ref), min(row[2], K)
    print(f"{form:22s} K={K:4d}  kernel e = {e_kernel:7.2f} u   fp32 F.linear e = {e_ref:6.2f} u   cap = {K + 8} u")


def softplus64(x):
    """softplus(beta = 1, threshold = 20) in fp64, overflow-free."""
    return torch.where(x > 20, x, torch.log1p(torch.exp(-x.abs())) + torch.clamp(x, min=0))


# ------------------------------------------------------------------------------------------------ value embedding
def _window(B, L, N, layout, g, scale=1.0):
    """``(flat, offset, strides)`` of an fp32 window [B, L, N] inside a flat buffer: ``plain`` contiguous and aligned,
    ``off1`` shifted by one element (rows no longer 16-byte aligned), ``view`` the last L rows of a longer [B, L+6, N],
    ``odd`` a batch stride of L*N + 1 elements."""
    T = L + 6 if layout == "view" else L
    bs = T * N + (1 if layout == "odd" else 0)
    off = (1 if layout == "off1" else 0) + (T - L) * N
    flat = torch.randn(off + B * bs, generator=g) * scale
    return flat, off, (bs, N, 1)


def _as_window(flat, off, strides, B, L, N):
    return torch.as_strided(flat, (B, L, N), strides, off)


def _embed_setup(ftn, dev, B, L, N, D, layout, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    flat, off, st = _window(B, L, N, layout, g, scale)
    w = torch.randn(D, N, generator=g) / N ** 0.5
    win = _as_window(flat, off, st, B, L, N)
    win_d, w_d = _as_window(flat.to(dev), off, st, B, L, N), w.to(dev)
    assert torch.equal(win_d.cpu(), win)
    form = ftn.runtime.embed_form(win_d, w_d)
    assert form == embed_rule(N, D, st[0] if B > 1 else 0, win_d.data_ptr() & 15, w_d.data_ptr() & 15, **SW_E)
    SEEN.add(form)
    return g, win, w, win_d, w_d, form


def _gemm_e(got, x, w, extra=0.0):
    """max over the elements of ``|got - x w^T| / (|x| |w|^T + extra)`` in u, and the fp64 product."""
    ref = x.double() @ w.double().t()
    den = x.double().abs() @ w.double().abs().t() + extra
    return float(((got.double() - ref).abs() / den).max()) / U, ref


def _check_embed(ftn, dev, B, L, N, D, layout, add_mode, ln_on, seed, want_default=None, scale=1.0):
    rt = ftn.runtime
    g, win, w, win_d, w_d, form = _embed_setup(ftn, dev, B, L, N, D, layout, seed, scale)
    if want_default is not None and DEFAULT_ENV:
        assert form == want_default
    # the GEMM alone
    got = rt.embed_forward(win_d, w_d, None, None).cpu()
    e, ref = _gemm_e(got, win, w)
    e_ref, _ = _gemm_e(Fn.linear(win.contiguous(), w), win, w)
    _record(form, N, e, e_ref)
    assert e <= N + 8, (form, e)
    # the epilogue: + add, LayerNorm
    add = None if add_mode is None else torch.randn(B if add_mode == "batch" else 1, L, D, generator=g) * scale
    lnp = ((torch.rand(D, generator=g) + 0.5), torch.randn(D, generator=g), 1e-5) if ln_on else None
    want = ref if add is None else ref + add.double()
    if lnp is not None:
        want = Fn.layer_norm(want, (D,), lnp[0].double(), lnp[1].double(), lnp[2])
    out = rt.embed_forward(win_d, w_d, None if add is None else add.to(dev),
                           None if lnp is None else (lnp[0].to(dev), lnp[1].to(dev), lnp[2]))
    np.testing.assert_allclose(out.cpu().numpy() / scale if lnp is None else out.cpu().numpy(),
                               (want / scale if lnp is None else want).numpy(), rtol=2e-5, atol=2e-5)
    return form


EMBED_FORM_CASES = [   # B, L, N, D, layout, add, LayerNorm, the form without switches
    (3, 24, 5, 8, "plain", "shared", False, "k_embed_in<4,false>"),
    (3, 24, 37, 128, "plain", "batch", True, "k_embed_in<8,false>"),        # D > 64, N % 4 != 0
    (2, 40, 64, 64, "plain", "shared", True, "k_embed_in_bf<4,2>"),
    (2, 40, 64, 128, "plain", "batch", False, "k_embed_in_bf<8,1>"),
    (3, 20, 64, 64, "off1", None, False, "k_embed_in<4,false>"),            # a "vector" N one element off
    (3, 20, 36, 128, "off1", "shared", True, "k_embed_in<8,false>"),
    (2, 24, 28, 36, "view", "batch", True, "k_embed_in_bf<4,2>"),           # batch stride (L + 6) N
    (3, 24, 200, 100, "view", "shared", False, "k_embed_in_bf<8,1>"),
    (3, 10, 8, 68, "odd", None, True, "k_embed_in<8,false>"),               # batch stride not a multiple of 4
    (3, 10, 512, 32, "odd", "batch", False, "k_embed_in<4,false>"),
    (1, 50, 60, 100, "odd", "shared", False, "k_embed_in_bf<8,1>"),         # B = 1: the stride is passed as 0
    (1, 50, 512, 64, "plain", None, True, "k_embed_in_bf<4,2>"),
]


@pytest.mark.parametrize("B,L,N,D,layout,add,ln,want", EMBED_FORM_CASES)
def test_embed_forms(B, L, N, D, layout, add, ln, want, ftn, dev):
    _check_embed(ftn, dev, B, L, N, D, layout, add, ln, seed=1000 + 7 * N + D, want_default=want)


_EDGE_N = [1, 3, 4, 8, 28, 36, 60, 64, 68, 100]
_EDGE_BL = [(1, 1), (3, 5), (2, 8), (1, 17), (7, 9), (4, 16), (5, 13), (1, 127), (3, 43), (37, 1)]   # B L = 1 ... 129


def _embed_edge_cases():
    """A pruned N x D product: every N with one d_model <= 64 and one > 64, aligned and one element off, so that each
    value meets each of the four forms it can reach; the row counts 1, 15, 16, 17, 63, 64, 65, 127, 129 and B = 37,
    L = 1 (the forecaster's per-step call) rotate through them, as do the epilogue variants."""
    out, i = [], 0
    for li, layout in enumerate(("plain", "off1")):
        for ni, N in enumerate(_EDGE_N):
            for D in ([4, 12, 36, 64][(ni + li) % 4], [68, 100, 128][(ni + li) % 3]):
                B, L = _EDGE_BL[(i * 3 + li) % 10]
                out.append((B, L, N, D, layout, [None, "shared", "batch"][i % 3], i % 2 == 0))
                i += 1
    return out


@pytest.mark.parametrize("B,L,N,D,layout,add,ln", _embed_edge_cases())
def test_embed_edges(B, L, N, D, layout, add, ln, ftn, dev):
    form = _check_embed(ftn, dev, B, L, N, D, layout, add, ln, seed=2000 + 131 * N + D)
    if DEFAULT_ENV:
        bf = layout == "plain" and N % 4 == 0
        assert form == (f"k_embed_in_bf<{4 if D <= 64 else 8},{2 if D <= 64 else 1}>" if bf
                        else f"k_embed_in<{4 if D <= 64 else 8},false>")


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("scale", [1e-12, 1e-6, 1.0, 1e6, 1e12])
def test_embed_input_scale(scale, D, ftn, dev):
    """Raw series values arrive at the bf16x3 embedding: ``e`` is scale-free, the same condition holds."""
    form = _check_embed(ftn, dev, 3, 23, 64, D, "plain", "shared", False, seed=3000 + D, scale=scale)
    assert not DEFAULT_ENV or form.startswith("k_embed_in_bf")


@pytest.mark.parametrize("N,D,layout", [(64, 64, "plain"), (36, 128, "plain"), (37, 36, "plain"), (64, 128, "off1")])
def test_embed_rows_strided_writes_only_its_rows(N, D, layout, ftn, dev):
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


@pytest.mark.parametrize("N,D,layout", [(64, 64, "plain"), (68, 128, "plain"), (37, 128, "plain"), (8, 12, "off1")])
def test_embed_row_isolation(N, D, layout, ftn, dev):
    """One NaN in x poisons its own output row and nothing else (bit for bit): a lane-map slip that averaged inputs
    hide moves the NaN into a neighbour's row."""
    rt = ftn.runtime
    B, L = 3, 23                                   # 69 rows: tiles straddle batch rows, the last one is partial
    g, win, w, win_d, w_d, form = _embed_setup(ftn, dev, B, L, N, D, layout, seed=5000 + N)
    add = torch.randn(1, L, D, generator=g).to(dev)
    clean = rt.embed_forward(win_d, w_d, add, None).cpu()
    for b, l, n in [(0, 0, 0), (1, 11, N // 2), (2, L - 1, N - 1)]:
        keep = win_d[b, l, n].clone()
        win_d[b, l, n] = float("nan")
        got = rt.embed_forward(win_d, w_d, add, None).cpu()
        win_d[b, l, n] = keep
        assert bool(got[b, l].isnan().all()), (form, b, l, n)
        got[b, l] = clean[b, l]
        assert torch.equal(got, clean), (form, b, l, n)


# ------------------------------------------------------------------------------------------------------ ring epilogue
@pytest.mark.parametrize("D", [4, 36, 64, 68, 128])
@pytest.mark.parametrize("B,L", [(1, 1), (1, 17), (5, 13)])
@pytest.mark.parametrize("mode", ["none", "shared", "batch_layer"])
def test_ring_against_fp64_and_the_one_pass_embedding(mode, B, L, D, ftn, dev):
    """``ftn_embed_ring`` at row counts 1, 17, 65 and heads 0, 1, L - 1: against fp64 (rolled V + add, LayerNorm) at the
    embedding's epilogue tolerance, and bit for bit against ``embed_forward`` of the rolled window."""
    rt = ftn.runtime
    N = 24 if D != 68 else 23                     # (d_model 68 on the fp32-MFMA form)
    g, win, w, win_d, w_d, form = _embed_setup(ftn, dev, B, L, N, D, "plain", seed=6000 + D + L)
    add = None if mode == "none" else torch.randn(B if mode == "batch_layer" else 1, L, D, generator=g)
    lnp = (torch.rand(D, generator=g) + 0.5, torch.randn(D, generator=g), 1e-5) if mode == "batch_layer" else None
    add_d = None if add is None else add.to(dev)
    ln_d = None if lnp is None else (lnp[0].to(dev), lnp[1].to(dev), lnp[2])
    V = torch.empty(B, L, D, device=dev)
    rt.embed_rows_strided(win_d, w_d, V, 0)
    for head in sorted({0, min(1, L - 1), L - 1}):
        got = rt.embed_ring(V, head, add_d, ln_d)
        want = torch.roll(V.cpu().double(), -head, dims=1)
        if add is not None:
            want = want + add.double()
        if lnp is not None:
            want = Fn.layer_norm(want, (D,), lnp[0].double(), lnp[1].double(), lnp[2])
        np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), rtol=2e-5, atol=2e-5)
        rolled = torch.roll(win_d, -head, dims=1).contiguous()
        one_pass = rt.embed_forward(rolled, w_d, add_d, ln_d)
        if lnp is not None and (D % 16 or form not in ftn.forecast.RING_EXACT_LAYER_FORMS):
            # the GEMM kernels contract the LayerNorm differently from k_embed_ring at a d_model that is not a multiple
            # of 16 and on some forms (k_embed_in<8, *>, k_embed_in_bf<8,2>): equal up to rounding; forecast.py keeps
            # everything outside RING_EXACT_LAYER_FORMS on the loop
            torch.testing.assert_close(got, one_pass, rtol=1e-5, atol=1e-5)
        else:
            assert torch.equal(got, one_pass), (form, head)


# -------------------------------------------------------------------------------------------------------------- heads
def _tail(B, hist, N, layout, g, dev):
    """fp32 tail [B, hist, N] and its device twin: ``plain`` the last rows of a longer window (an aligned view when
    N % 4 == 0), ``off1`` one element off, ``odd`` a batch stride that is not a multiple of 4."""
    T = hist + 5
    bs = T * N + (1 if layout == "odd" else 0)
    off = (1 if layout == "off1" else 0) + (T - hist) * N
    flat = 3.0 * torch.randn(off + B * bs, generator=g)
    t = torch.as_strided(flat, (B, hist, N), (bs, N, 1), off)
    return t, torch.as_strided(flat.to(dev), (B, hist, N), (bs, N, 1), off)


def _head_ref(hidden, w_mu, b_mu, w_sg, b_sg, tail, S, late, floor):
    """The heads in fp64 (the softplus included): ``floor`` a float or an [N] tensor."""
    d = lambda t: t.double()
    hist = tail.shape[1]
    tf = d(tail) if hist == S else torch.cat([d(tail), d(tail)[:, -1:].expand(-1, S - hist, -1)], dim=1)
    pre = d(hidden) @ d(w_mu).t() + d(b_mu) + tf
    if late is not None:
        pre = pre + d(late)
    sg = d(hidden) @ d(w_sg).t() + d(b_sg)
    fl = d(floor) if isinstance(floor, torch.Tensor) else float(np.float32(floor))
    return softplus64(pre) + 1e-6, softplus64(sg) + fl + 1e-6


def _check_heads(ftn, dev, B, S, D, N, hist, layout, late_mode, floor_mode, seed, want_default=None, measure=True,
                 need_loop=False):
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
    assert (form, cap) == head_rule(N, D, tail_d.stride(0) if B > 1 else 0, late_bs, tail_d.data_ptr() & 15, **SW_H)
    SEEN.add(form)
    if want_default is not None and DEFAULT_ENV:
        assert form == want_default
    if need_loop:
        assert B * S > 64 * cap and (B * S - 64 * cap) % 16 != 0, (form, cap)      # the row loop iterates, ragged end
    # the whole operation
    rate, disp, bad = rt.head_forward(hd, wm, to(b_mu), ws, to(b_sg), tail_d, hist, to(late), to(fv), 1e-3)
    want_r, want_d = _head_ref(hidden, w_mu, b_mu, w_sg, b_sg, tail, S, late, fv if fv is not None else 1e-3)
    assert int(bad.item()) == 0
    np.testing.assert_allclose(rate.cpu().numpy(), want_r.numpy(), rtol=2e-5, atol=1e-6)
    np.testing.assert_allclose(disp.cpu().numpy(), want_d.numpy(), rtol=2e-5, atol=1e-6)
    if not measure:
        return form
    # the two GEMMs alone: where pre > 20 the softplus is the identity and rate - 1e-6 is the pre-activation.  hidden
    # is scaled to get there (a large bias would enter the denominator and dilute a lost product); tail (zeroed in
    # place: same view, same form), late and biases are 0.  At least 256 rows, so that enough elements qualify.
    Sm = max(S, 256 // B + 1)
    hidden = torch.randn(B, Sm, D, generator=g)
    zero_n = torch.zeros(N, device=dev)
    tail_d.zero_()
    assert rt.head_form(to(hidden), wm, tail_d, None)[0] == head_rule(N, D, tail_d.stride(0) if B > 1 else 0, 0,
                                                                        tail_d.data_ptr() & 15, **SW_H)[0] == form
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
        lin = Fn.linear(h30, w).double()
        e_ref = float(((lin - ref).abs() / den)[past].max()) / U
        _record(form, D, e, e_ref)
        assert e <= D + 8, (form, name, e)
    return form


_HEAD_D = [4, 12, 16, 20, 32, 36, 48, 64, 68, 100, 128]
_HEAD_N_VEC = [8, 60, 64, 68, 200]
_HEAD_N_ANY = [1, 5, 8, 60, 64, 68, 200]
_HEAD_BS = [(3, 6, 6), (2, 12, 12), (4, 5, 3), (2, 1, 1), (1, 24, 24), (5, 7, 2)]   # B, S, hist (hist < S: edge-padded)


def _head_cases():
    """Every d_model on its vector form (k_head_bf, or k_head<*, true> under FTN_HEAD_F32=1) and on its scalar form:
    N % 4 != 0, or a vector N behind a tail that is one element off or has an odd batch stride."""
    out = []
    for i, D in enumerate(_HEAD_D):
        N = _HEAD_N_VEC[i % 5]
        B, S, hist = _HEAD_BS[i % 6]
        nt_ns = "4,1" if D <= 32 else "4,2" if D <= 64 else "2,4"
        out.append((B, S, D, N, hist, "plain", [None, "shared", "batch"][i % 3], ["scalar", "vector"][i % 2],
                    f"k_head_bf<{nt_ns}>"))
        N = _HEAD_N_ANY[(i * 3) % 7]
        B, S, hist = _HEAD_BS[(i + 2) % 6]
        layout = "plain" if N % 4 else ("off1" if i % 2 else "odd")
        if layout == "odd" and B == 1:
            layout = "off1"                            # (the stride of a one-row batch is passed as 0)
        ns = 1 if D <= 16 else 2 if D <= 32 else 4 if D <= 64 else 8
        out.append((B, S, D, N, hist, layout, [None, "shared", "batch"][(i + 1) % 3], ["scalar", "vector"][(i + 1) % 2],
                    f"k_head<{ns},false>"))
    return out


@pytest.mark.parametrize("B,S,D,N,hist,layout,late,floor,want", _head_cases())
def test_head_forms(B, S, D, N, hist, layout, late, floor, want, ftn, dev):
    _check_heads(ftn, dev, B, S, D, N, hist, layout, late, floor, seed=7000 + 13 * D + N, want_default=want)


@pytest.mark.parametrize("B,S,D,layout,want", [
    (7, 9400, 16, "odd", "k_head<1,false>"),          # 65 800 rows > 64 x 1024
    (3, 16500, 16, "plain", "k_head_bf<4,1>"),        # 49 500 rows > 64 x 768
    (3, 16500, 64, "plain", "k_head_bf<4,2>"),
    (3, 8300, 128, "plain", "k_head_bf<2,4>"),        # 24 900 rows > 64 x 384 (two series tiles)
])
def test_head_row_loop(B, S, D, layout, want, ftn, dev):
    """Rows beyond 64 x the gridDim.y cap by a non-multiple of 16: a workgroup walks several row tiles and the last
    tile is partial.  Every row is compared."""
    _check_heads(ftn, dev, B, S, D, 64, 4, layout, "shared" if D == 16 else None, "vector", seed=8000 + D,
                 want_default=want, measure=False, need_loop=True)


@pytest.mark.parametrize("D,N,layout", [(16, 8, "plain"), (64, 5, "plain"), (128, 64, "plain"), (32, 64, "off1")])
def test_head_row_isolation(D, N, layout, ftn, dev):
    """One NaN in ``hidden`` poisons both outputs of its own row only and raises both bits of the flag, on the fp32
    and on the 16-bit forms."""
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


def _sweep_points():
    """A dense grid over [-104, 25] and the seams of softplus20's three branches: 20 and its fp32 neighbours,
    |x| = 6 ln 2 (where exp(-|x|) = 2^-6 switches series and log2 form) and its neighbours, 0, +-tiny."""
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)
    seams = []
    for c in (20.0, 6 * np.log(2.0), -6 * np.log(2.0)):
        x = f32([c])
        lo = hi = x
        seams.append(x)
        for _ in range(8):
            lo, hi = torch.nextafter(lo, f32([-1e9])), torch.nextafter(hi, f32([1e9]))
            seams += [lo, hi]
    seams.append(f32([0.0, -0.0, 1e-30, -1e-30, 1e-42, -1e-42, 1e-7, -1e-7, 25.0, -104.0, -87.3, -88.8, -103.9]))
    seams = torch.cat(seams)
    n = 1 << 18
    grid = torch.linspace(-104.0, 25.0, n - seams.numel(), dtype=torch.float64).float()
    return torch.cat([grid, seams])


def _ulps(got, ref):
    """|got - ref| in units of 2^-23 of the result (the unit the fp32 torch softplus measures 0.96 in)."""
    return ((got.double() - ref).abs() / (ref.abs() * 2.0 ** -23))


def test_softplus_sweep(ftn, dev):
    """``softplus20`` through both heads with the pre-activation carried exactly (hidden = 0, biases 0): by ``tail`` for
    the rate, by ``b_sigma`` of a one-row batch for the dispersion.  Reference: fp64
    ``where(x > 20, x, log1p(exp(-|x|)) + max(x, 0)) + 1e-6`` on the same fp32 x.  Limit: 4 ulp (2^-23 relative) of the
    result - one each for the hardware exp2 and log2, the log2(e) / ln 2 scalings and the final sums of positive
    terms.  Measured on the MI355X: 1.92 ulp for both heads (31.7 ulp before the two roundings in softplus20 were
    compensated); torch's fp32 softplus on the CPU measures 1.36 ulp over the same points."""
    rt = ftn.runtime
    x = _sweep_points()
    n, N = x.numel(), 64
    ref = softplus64(x.double()) + 1e-6
    e_torch = float(_ulps(Fn.softplus(x, 1.0, 20.0) + 1e-6, ref).max())
    # rate: rows of 64 series, the value in tail
    S = n // N
    zw, zb = torch.zeros(N, 4, device=dev), torch.zeros(N, device=dev)
    tail = x.view(1, S, N).to(dev)
    SEEN.add(rt.head_form(torch.zeros(1, S, 4, device=dev), zw, tail)[0])
    rate, disp, bad = rt.head_forward(torch.zeros(1, S, 4, device=dev), zw, zb, zw, zb, tail, S, None, None, 0.0)
    assert int(bad.item()) == 0
    rate = rate.cpu().reshape(-1)
    e_rate = _ulps(rate, ref)
    assert bool((rate > 0).all()) and bool((disp > 0).all())
    # dispersion: one row, the value in b_sigma, floor 0
    zw1 = torch.zeros(n, 4, device=dev)
    t1 = torch.zeros(1, 1, n, device=dev)
    SEEN.add(rt.head_form(torch.zeros(1, 1, 4, device=dev), zw1, t1)[0])
    r1, d1, bad1 = rt.head_forward(torch.zeros(1, 1, 4, device=dev), zw1, torch.zeros(n, device=dev), zw1, x.to(dev),
                                   t1, 1, None, None, 0.0)
    assert int(bad1.item()) == 0
    d1 = d1.cpu().reshape(-1)
    e_disp = _ulps(d1, ref)
    assert bool((d1 > 0).all()) and bool((r1 > 0).all())
    worst = int(torch.argmax(torch.maximum(e_rate, e_disp)))
    print(f"softplus20: rate {float(e_rate.max()):.2f} ulp, dispersion {float(e_disp.max()):.2f} ulp "
          f"(worst at x = {float(x[worst])!r}); torch fp32 softplus {e_torch:.2f} ulp")
    E_TABLE["softplus20"] = [max(float(e_rate.max()), float(e_disp.max())), e_torch, 0]
    assert float(e_rate.max()) <= 4.0 and float(e_disp.max()) <= 4.0, (float(e_rate.max()), float(e_disp.max()),
                                                                      float(x[worst]))


def test_head_flag_bits_separately(ftn, dev):
    """+inf in ``tail`` raises bit 0 only, a NaN in ``b_sigma`` bit 1 only."""
    rt = ftn.runtime
    B, S, D, N = 2, 5, 8, 16
    g = torch.Generator().manual_seed(11)
    hidden, w = torch.randn(B, S, D, generator=g).to(dev), torch.randn(N, D, generator=g).to(dev)
    b, tail = torch.zeros(N, device=dev), torch.randn(B, S, N, generator=g).to(dev)
    bad_tail = tail.clone()
    bad_tail[1, 2, 3] = float("inf")
    assert int(rt.head_forward(hidden, w, b, w, b, bad_tail, S, None, None, 1e-3)[2].item()) == 1
    bad_b = b.clone()
    bad_b[7] = float("nan")
    assert int(rt.head_forward(hidden, w, b, w, bad_b, tail, S, None, None, 1e-3)[2].item()) == 2
    assert int(rt.head_forward(hidden, w, b, w, b, tail, S, None, None, 1e-3)[2].item()) == 0


# ------------------------------------------------------------------------------------------------- residual LayerNorm
@pytest.mark.parametrize("C", [1, 7, 64, 128, 512, 513, 700])
def test_residual_layernorm(C, ftn, dev):
    """``k_resid_ln`` across its register-cached part (C <= 512) and its re-reading tail, rows that do not fill a
    workgroup, in place and out of place (identical bits), against fp64 ``layer_norm(x + (new - x))``."""
    rt = ftn.runtime
    g = torch.Generator().manual_seed(C)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    for rows in (1, 3, 4, 5, 1001):
        x, new = torch.randn(rows, C, generator=g), torch.randn(rows, C, generator=g)
        want = Fn.layer_norm(x.double() + (new.double() - x.double()), (C,), gamma.double(), beta.double(), 1e-5)
        xd, nd = x.to(dev), new.to(dev)
        out = rt.residual_layernorm(xd, nd, gamma.to(dev), beta.to(dev), 1e-5)
        assert torch.equal(nd.cpu(), new)
        inplace = rt.residual_layernorm(xd, nd, gamma.to(dev), beta.to(dev), 1e-5, out=nd)
        assert inplace.data_ptr() == nd.data_ptr() and torch.equal(inplace, out), (C, rows)
        if C == 1:
            assert torch.equal(out.cpu(), beta.expand(rows, 1))
        else:
            np.testing.assert_allclose(out.cpu().numpy(), want.numpy(), rtol=1e-5, atol=2e-6)


# ------------------------------------------------------------------------------- recursive forecast of a misaligned view
@pytest.mark.parametrize("d_model", [64, 128])
@pytest.mark.parametrize("norm", ["none", "layer"])
def test_misaligned_recursive_forecast_equals_the_loop(norm, d_model, ftn, dev):
    """``last_seq`` as a view one element into a buffer (N % 4 == 0): its first window runs the fp32-MFMA embedding,
    every later window of the reference loop is a fresh aligned tensor on the bf16x3 form.  The forecast must still be
    ``torch.equal`` to the loop over the same model."""
    from test_gpu_recursive import _inputs, _loop, _model

    N, L, T, B, H = 32, 16, 20, 3, 20
    model = _model(ftn, dev, d_model, N, L, 0, norm)
    x0, kw = _inputs(dev, B, T, N, H, 0, seed=5)
    flat = torch.zeros(1 + B * T * N, device=dev)
    x = flat[1:].view(B, T, N)
    x.copy_(x0)
    assert x.data_ptr() % 16 == 4
    w = model.embedding.value_embedding.weight
    first, later = ftn.runtime.embed_form(x[:, -L:], w), ftn.runtime.embed_form(x0[:, -L:], w)
    assert first == embed_rule(N, d_model, T * N, 4, 0, **SW_E) and later == embed_rule(N, d_model, T * N, 0, 0, **SW_E)
    with torch.inference_mode():
        want_r, want_d = _loop(model, x, H, **kw)
        got_r, got_d = ftn.forecast.forecast_recursive_batch(model, x, H, **kw)
        # the aligned copy still takes the device path and equals its own loop
        al_r, al_d = ftn.forecast.forecast_recursive_batch(model, x0, H, **kw)
        alw_r, alw_d = _loop(model, x0, H, **kw)
    torch.cuda.synchronize()
    assert torch.equal(got_r, want_r) and torch.equal(got_d, want_d)
    assert torch.equal(al_r, alw_r) and torch.equal(al_d, alw_d)


def test_layer_mode_forecast_at_ragged_d_model_equals_the_loop(ftn, dev):
    """"layer" mode at a d_model that is not a multiple of 16: ring and one-pass embedding agree up to rounding only
    (the case above), so the forecast must not come from the ring."""
    from test_gpu_recursive import _inputs, _loop, _model

    N, L, T, B, H = 32, 16, 20, 3, 12
    model = _model(ftn, dev, 36, N, L, 0, "layer")
    x, kw = _inputs(dev, B, T, N, H, 0, seed=7)
    with torch.inference_mode():
        want_r, want_d = _loop(model, x, H, **kw)
        got_r, got_d = ftn.forecast.forecast_recursive_batch(model, x, H, **kw)
    torch.cuda.synchronize()
    assert model._last_embed_backend == "hip" and model._last_head_backend == "hip"
    assert torch.equal(got_r, want_r) and torch.equal(got_d, want_d)


# ---------------------------------------------------------------------------------------------------- what ran (last)
def test_every_form_ran():
    """Every form the library can reach under the current switches was run (and compared) by the cases above."""
    no_rt = lambda no: SW_E["rt"] if SW_E["rt"] in (1, 2) else (2 if no == 4 else 1)
    want = {f"k_embed_in<{no},false>" for no in (4, 8)} | {f"k_head<{ns},false>" for ns in (1, 2, 4, 8)}
    want |= ({f"k_embed_in<{no},true>" for no in (4, 8)} if SW_E["f32"] else
             {f"k_embed_in_bf<{no},{no_rt(no)}>" for no in (4, 8)})
    want |= ({f"k_head<{ns},true>" for ns in (1, 2, 4, 8)} if SW_H["f32"] else
             {"k_head_bf<4,1>", "k_head_bf<4,2>", "k_head_bf<2,4>"})
    print("\nform                    min K   kernel e [u]   fp32 F.linear e [u]")
    for form in sorted(E_TABLE):
        k, r, K = E_TABLE[form]
        print(f"{form:22s} {K:6d} {k:14.2f} {r:21.2f}")
    assert want <= SEEN, sorted(want - SEEN)
    # every 16-bit form was measured at K <= 128 somewhere (the heads always; the embedding by its edge cases)
    assert all(f in E_TABLE and E_TABLE[f][2] <= 128 for f in want), sorted(want - set(E_TABLE))
