"""The context front end on the MI355X (``ftn_context_rows``, ``ftn_context_through_weight``, ``ftn_embed_add``:
csrc/context.hip) against an fp64 restatement of the shell's torch ops, then the whole model in the pipeline layout
and against its CPU mirror.

Metric, as in ``test_gpu_shell_wide.py``: ``e = |got - ref64| / sum|terms|`` in units of u = 2^-24, per output.  The
cap of an output is not a constant: it is the first-order rounding budget of the fp32 chain that produced it,
propagated through the stages in fp64 next to the reference (``_lin``, ``_ln`` below), times ``SLACK`` for the
second-order terms:

* a dot product of n terms is one chain of n FMAs from +0 and one more addition for the bias: ``(n + 1) u sum|terms|``;
* a LayerNorm over n values (mean m, deviations d, sigma = sqrt(var + eps), z = |d| / sigma, kappa = mean|x| / sigma):
  each of the two reductions is a tree of depth T (a lane's slots, then the 6 steps of the wave butterfly) and a
  division, so |dm| <= (T + 1) u mean|x|, |dd| <= u ((T + 3) mean|x| + |d|), the variance is off by
  (T + 5 + 2 (T + 3) kappa) u relative (all its terms are positive, each square rounded once; sum|d| / sum d^2 <=
  1 / sigma), 1 / sqrt(var + eps) by half of that + 3 u (the addition of eps, the square root, the division), the
  two products of the affine part by 2 u and its addition by u |y|:
  ``|dy| <= u (|g| ((T + 3) kappa (1 + z) + z (T / 2 + 9)) + |y|)``; an error dx of the inputs arrives as
  ``|g| / sigma (|dx| + mean|dx| + z mean(z |dx|))`` (the Jacobian of the normalisation);
* a sum of two values adds u of the result.

For a LayerNorm output ``sum|terms| = |g| (kappa (1 + z) + z) + |b|``.  Measured on the MI355X (``-s`` prints every
case): the largest e of a kernel, the cap of the element it occurred at, and the largest ``|err| / budget`` anywhere:
    k_context_rows   rows 8.4 u (cap 1432 u, 0.12 of the budget)   coeff 3.2 u (2502 u, 0.06)
                     cbias 3.8 u (324 u, 0.04)                     late 3.7 u (170 u, 0.03)
    k_through_small  5.2 u at N = 64 (cap 64 u); N = 1 is one rounding, 0.995 of its 1 u
    k_through_chunks 1.7 u at N = 513 (cap 194 u)
    k_embed_add      none 4.0 u (cap 7.6 u; a single addition reaches 1.000 of its 1 u)   decoupled 3.6 u (cap 22.8 u, 0.99)
    pipeline fixture 0.7 % of rtol 1e-4 / atol 2e-5; model against its fp32 CPU mirror at most 3.2 % (d_model 192, direct)
"""
import json

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_predict_pipeline_dropin import MODEL as PIPE_MODEL, _part

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
SLACK = 1.0 + 1e-3           # the budgets are first order in u
RTOL, ATOL = 1e-4, 2e-5      # the GPU suite's model tolerance
GUARD = 64                   # sentinel floats on either side of an output
SENT = -7.25e7
E_MAX = {}                   # output name -> (largest e, the cap of that element)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a ROCm device"
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------ fp64 reference with its budget
def _lin(x, dx, W, b):
    """``x W^T + b`` in fp64, its sum|terms|, and the budget: the inputs' error through |W| + (n + 1) u sum|terms|."""
    W, b = W.double(), b.double()
    y = x @ W.T + b
    terms = x.abs() @ W.abs().T + b.abs()
    return y, dx @ W.abs().T + (x.shape[-1] + 1) * U * terms, terms


def _ln(x, dx, g, b, eps, T):
    """Affine LayerNorm over the last axis in fp64, budget and sum|terms| as derived in the module docstring."""
    g, b = g.double(), b.double()
    d = x - x.mean(-1, keepdim=True)
    sig = (d.square().mean(-1, keepdim=True) + eps).sqrt()
    z, kappa = d.abs() / sig, x.abs().mean(-1, keepdim=True) / sig
    y = g * d / sig + b
    own = U * (g.abs() * ((T + 3) * kappa * (1 + z) + z * (T / 2 + 9)) + y.abs())
    prop = g.abs() / sig * (dx + dx.mean(-1, keepdim=True) + z * (z * dx).mean(-1, keepdim=True))
    return y, own + prop, g.abs() * (kappa * (1 + z) + z) + b.abs()


def _measure(name, got, ref, budget, terms):
    """Assert ``|got - ref| <= SLACK budget`` element by element; print, and keep per kernel, the largest e and the
    cap of the element it occurred at, in units of u."""
    err = (got.detach().cpu().double() - ref).abs()
    eu, capu = (err / (U * terms)).flatten(), (budget / (U * terms)).flatten()
    at = int(eu.argmax())
    e, cap, worst = float(eu[at]), float(capu[at]), float((err / budget).max())
    if e >= E_MAX.get(name, (-1.0, 0.0))[0]:
        E_MAX[name] = (e, cap)
    print(f"{name:22s} max e = {e:6.2f} u (cap there {cap:7.2f} u)   worst |err| / budget = {worst:.3f}")
    assert torch.isfinite(got).all()
    assert worst <= SLACK, (name, e, cap, worst)


def _guarded(dev, *shape):
    """A contiguous fp32 output in the middle of a sentinel-filled buffer, 16-byte aligned."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENT, dtype=torch.float32, device=dev)
    return buf, buf[GUARD:GUARD + n].view(*shape)


def _guards_intact(buf):
    return bool((buf[:GUARD] == SENT).all()) and bool((buf[-GUARD:] == SENT).all())


def _off1(t, dev):
    """``t`` on the device, one float past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev)
    assert buf.data_ptr() % 16 == 0
    out = buf[1:].view(t.shape)
    out.copy_(t)
    return out


# ----------------------------------------------------------------------------------------------------- series rows
def _row_params(g, F, Ws, Ed, V, R, steps, static_ln):
    ctx = Ws + Ed
    rn = lambda *s, sc=1.0: sc * torch.randn(*s, generator=g)
    P = dict(F=F, Ws=Ws, Ed=Ed, V=V, R=R, steps=steps, ctx=ctx, static_ln=static_ln)
    if Ws:
        P.update(w_s=rn(Ws, F, sc=F ** -0.5), b_s=rn(Ws, sc=0.3), sn_g=1 + rn(Ws, sc=0.2), sn_b=rn(Ws, sc=0.2))
    if Ed:
        P.update(emb=rn(V, Ed))
    P.update(cn_g=1 + rn(ctx, sc=0.2), cn_b=rn(ctx, sc=0.2), w_c=rn(R, ctx, sc=ctx ** -0.5), b_c=rn(R, sc=0.2),
             w_p=rn(1, ctx, sc=ctx ** -0.5), b_p=rn(1, sc=0.2), ln_g=1 + rn(ctx, sc=0.2), ln_b=rn(ctx, sc=0.2),
             w_l=rn(steps, ctx, sc=ctx ** -0.5), b_l=rn(steps, sc=0.2), gate=0.05 + rn(steps, sc=0.02))
    return P


def _rows_ref(P, static, ids):
    """fp64 restatement of ``_rows_of`` + ``_context_terms`` + ``_late_bias`` for static [Bc, N, F], ids [Bc, N]."""
    slots = lambda n: -(-n // 64) + 6
    cols, dcols = [], []
    if P["Ws"]:
        s, ds, _ = _lin(static.double(), torch.zeros_like(static, dtype=torch.float64), P["w_s"], P["b_s"])
        if P["static_ln"]:
            s, ds, _ = _ln(s, ds, P["sn_g"], P["sn_b"], 1e-5, slots(P["Ws"]))
        cols.append(s)
        dcols.append(ds)
    if P["Ed"]:
        e = P["emb"].double()[ids]
        cols.append(e)
        dcols.append(torch.zeros_like(e))
    c, dc, tc = _ln(torch.cat(cols, -1), torch.cat(dcols, -1), P["cn_g"], P["cn_b"], 1e-5, slots(P["ctx"]))
    coeff = _lin(c, dc, P["w_c"], P["b_c"])
    cb = tuple(t.squeeze(-1) for t in _lin(c, dc, P["w_p"], P["b_p"]))
    ln, dln, _ = _ln(c, dc, P["ln_g"], P["ln_b"], 1e-5, slots(P["ctx"]))
    lb, dlb, tlb = _lin(ln, dln, P["w_l"], P["b_l"])
    gt = P["gate"].double()
    late = tuple(t.transpose(1, 2) for t in (gt * lb, gt.abs() * dlb + U * (gt * lb).abs(), gt.abs() * tlb))
    return dict(rows=(c, dc, tc), coeff=coeff, cbias=cb, late=late)


def _rows_run(ftn, dev, P, static, ids, Bc, N, want=("rows", "coeff", "cbias", "late"), off1=False, put=None):
    """``runtime.context_rows`` into guarded outputs; ``static`` / ``ids`` as the caller lays them out (device)."""
    put = put or ((lambda t: _off1(t, dev)) if off1 else (lambda t: t.to(dev)))
    D = {k: put(v) for k, v in P.items() if isinstance(v, torch.Tensor)}
    shapes = dict(rows=(Bc, N, P["ctx"]), coeff=(Bc, N, P["R"]), cbias=(Bc, N), late=(Bc, P["steps"], N))
    bufs = {k: _guarded(dev, *shapes[k]) for k in want}
    kw = {}
    if P["Ws"]:
        kw.update(static=static, static_proj=(D["w_s"], D["b_s"]),
                  static_norm=(D["sn_g"], D["sn_b"], 1e-5) if P["static_ln"] else None)
    if P["Ed"]:
        kw.update(ids=ids, table=D["emb"])
    ftn.runtime.context_rows(
        Bc, N, (D["cn_g"], D["cn_b"], 1e-5), coeff=(D["w_c"], D["b_c"]) if "coeff" in want else None,
        proj=(D["w_p"], D["b_p"]) if "cbias" in want else None,
        late=((D["ln_g"], D["ln_b"], 1e-5), D["w_l"], D["b_l"], D["gate"]) if "late" in want else None,
        want_rows="rows" in want, out=tuple(bufs[k][1] if k in want else None for k in ("rows", "coeff", "cbias", "late")),
        **kw)
    torch.cuda.synchronize()
    assert all(_guards_intact(b) for b, _ in bufs.values()), "bytes around an output changed"
    return {k: v.clone() for k, (_, v) in bufs.items()}


def _row_inputs(g, P, Bc, N):
    static = torch.randn(Bc, N, P["F"], generator=g) + 0.5
    ids = torch.randint(0, P["V"], (Bc, N), generator=g)          # repeated, non-monotone
    return static, ids


ROW_CASES = [   # Ws, Ed, F, static_layernorm, R, steps, N, Bc, inputs one float off a 16-byte boundary
    (5, 6, 7, True, 3, 7, 5, 3, False), (5, 6, 1, False, 32, 96, 1, 3, True), (0, 32, 1, True, 1, 1, 1, 1, False),
    (0, 32, 7, True, 3, 96, 70, 3, True), (16, 0, 1, False, 32, 96, 70, 1, False), (16, 0, 64, True, 3, 7, 5, 1, True),
    (64, 32, 64, True, 3, 7, 5, 3, False), (64, 32, 7, False, 1, 1, 70, 1, True),
    (128, 128, 64, True, 32, 96, 5, 1, True), (128, 128, 7, False, 1, 1, 70, 3, False)]


@pytest.mark.parametrize("Ws,Ed,F,sln,R,steps,N,Bc,off1", ROW_CASES)
def test_rows_against_fp64(Ws, Ed, F, sln, R, steps, N, Bc, off1, ftn, dev):
    g = torch.Generator().manual_seed(100 + Ws + Ed + F + R + N)
    P = _row_params(g, F, Ws, Ed, 9, R, steps, sln)
    static, ids = _row_inputs(g, P, Bc, N)
    st_d = _off1(static, dev) if off1 else static.to(dev)
    got = _rows_run(ftn, dev, P, st_d, ids.to(dev), Bc, N, off1=off1)
    again = _rows_run(ftn, dev, P, st_d, ids.to(dev), Bc, N, off1=off1)
    assert all(torch.equal(got[k], again[k]) for k in got), "two runs differ"
    ref = _rows_ref(P, static, ids)
    for k in ("rows", "coeff", "cbias", "late"):
        _measure(k, got[k], *ref[k])


@pytest.mark.parametrize("want", [("rows",), ("coeff",), ("cbias",), ("late",), ("coeff", "late"), ("rows", "cbias")])
def test_rows_optional_outputs(want, ftn, dev):
    """Each output alone (and two pairs) holds the bits it has beside all the others."""
    g = torch.Generator().manual_seed(7)
    P = _row_params(g, 7, 5, 6, 9, 3, 7, True)
    static, ids = (t.to(dev) for t in _row_inputs(g, P, 3, 5))
    full = _rows_run(ftn, dev, P, static, ids, 3, 5)
    part = _rows_run(ftn, dev, P, static, ids, 3, 5, want=want)
    assert set(part) == set(want) and all(torch.equal(part[k], full[k]) for k in want)


@pytest.mark.parametrize("Ws,Ed", [(5, 6), (64, 32), (0, 32), (128, 128)])
def test_row_invariance(Ws, Ed, ftn, dev):
    """A row's bits do not depend on Bc, on N, on which rows share the call, or on whether ids / statics were given
    once or per sample."""
    g = torch.Generator().manual_seed(11 + Ws)
    B, N = 3, 70
    P = _row_params(g, 7, Ws, Ed, 9, 3, 7, True)
    s1, i1 = (t.to(dev) for t in _row_inputs(g, P, 1, N))
    shared = _rows_run(ftn, dev, P, s1[0], i1[0], 1, N)                       # [N, F] statics, [N] ids
    per = _rows_run(ftn, dev, P, s1.expand(B, -1, -1).contiguous(), i1.expand(B, -1).contiguous(), B, N)
    for k in shared:
        assert all(torch.equal(per[k][b], shared[k][0]) for b in range(B)), k
    # different rows per sample: a column slice [off, off + n) of the batch, and one sample alone
    sb, ib = (t.to(dev) for t in _row_inputs(g, P, B, N))
    full = _rows_run(ftn, dev, P, sb, ib, B, N)
    off, n = 13, 5
    part = _rows_run(ftn, dev, P, sb[:, off:off + n], ib[:, off:off + n], B, n)       # strided views, not copies
    assert not sb[:, off:off + n].is_contiguous()
    assert torch.equal(part["rows"], full["rows"][:, off:off + n]) and torch.equal(part["coeff"], full["coeff"][:, off:off + n])
    assert torch.equal(part["cbias"], full["cbias"][:, off:off + n]) and torch.equal(part["late"], full["late"][:, :, off:off + n])
    one = _rows_run(ftn, dev, P, sb[1:2], ib[1:2], 1, N)
    assert all(torch.equal(one[k][0], full[k][1]) for k in one)


@pytest.mark.parametrize("bad_id", [9, -1, 2 ** 40])
def test_out_of_range_id_gives_nan_in_that_row_only(bad_id, ftn, dev):
    """The kernel compares the id with the table's size and reads nothing for it: no fault is involved."""
    g = torch.Generator().manual_seed(5)
    P = _row_params(g, 7, 5, 6, 9, 3, 7, True)
    static, ids = _row_inputs(g, P, 3, 5)
    clean = _rows_run(ftn, dev, P, static.to(dev), ids.to(dev), 3, 5)
    ids[1, 3] = bad_id
    got = _rows_run(ftn, dev, P, static.to(dev), ids.to(dev), 3, 5)
    hit = torch.zeros(3, 5, dtype=torch.bool, device=dev)
    hit[1, 3] = True
    for k, mask in (("rows", hit[..., None]), ("coeff", hit[..., None]), ("cbias", hit), ("late", hit[:, None, :])):
        mask = mask.expand_as(got[k])
        assert torch.isnan(got[k][mask]).all() and torch.equal(got[k][~mask], clean[k][~mask]), k


# --------------------------------------------------------------------------------------------------- through-weight
def _chain(N):
    """The longest chain of additions of an output: N FMAs up to 64 series; beyond, the chunks of one of the four
    parts and the two additions of the tree."""
    return N if N <= 64 else -(-(-(-N // 64)) // 4) * 64 + 2


@pytest.mark.parametrize("N", [1, 3, 64, 513, 4096])
def test_through_weight_against_fp64(N, ftn, dev):
    g = torch.Generator().manual_seed(N)
    name = "k_through_small" if N <= 64 else "k_through_chunks"
    for D in (16, 132, 512):
        wide = torch.randn(D, N + 5, generator=g) / N ** 0.5
        w_d = wide.to(dev)[:, 2:2 + N]                                   # a strided column slice
        w = wide[:, 2:2 + N].double()
        for R, Bc in ((1, 1), (1, 3), (32, 1), (32, 3)):
            coeff, cbias = torch.randn(Bc, N, R, generator=g), torch.randn(Bc, N, generator=g)
            (bq, qc), (bb, qb) = _guarded(dev, Bc, R, D), _guarded(dev, Bc, D)
            ftn.runtime.context_through_weight(coeff.to(dev), cbias.to(dev), w_d, out=(qc, qb))
            torch.cuda.synchronize()
            assert _guards_intact(bq) and _guards_intact(bb)
            tq = torch.einsum("bnr,dn->brd", coeff.double().abs(), w.abs())
            tb = cbias.double().abs() @ w.abs().T
            _measure(name, qc, torch.einsum("bnr,dn->brd", coeff.double(), w), _chain(N) * U * tq, tq)
            _measure(name, qb, cbias.double() @ w.T, _chain(N) * U * tb, tb)
            # either output alone, and a batch row alone: the same bits
            only_c, _ = ftn.runtime.context_through_weight(coeff.to(dev), None, w_d)
            _, only_b = ftn.runtime.context_through_weight(None, cbias.to(dev), w_d)
            assert torch.equal(only_c, qc) and torch.equal(only_b, qb)
            if Bc > 1:
                c1, b1 = ftn.runtime.context_through_weight(coeff[1:2].to(dev), cbias[1:2].to(dev), w_d)
                assert torch.equal(c1[0], qc[1]) and torch.equal(b1[0], qb[1])
                cw, _ = ftn.runtime.context_through_weight(coeff.to(dev), None, w_d.contiguous())
                assert torch.equal(cw, qc)                               # the row stride does not change the bits


# -------------------------------------------------------------------------------------------------------- embed-add
def _add_ref(A, L, D, T, mode, mark, epi, qc, qb):
    """fp64 ``add`` [Ba, L, D] with its budget; the terms in the order ``_through_weight`` documents."""
    Ba = max(1 if mark is None else mark.shape[0], 1 if qc is None else qc.shape[0], 1 if qb is None else qb.shape[0])
    t = torch.zeros(Ba, L, D, dtype=torch.float64)
    dt, terms = torch.zeros_like(t), torch.zeros_like(t)
    if epi:
        aux = A["pos"].double().expand(Ba, L, D).clone()
        daux, taux = torch.zeros_like(aux), aux.abs()
        if T:
            m, dm, tm = _lin(mark.double().expand(Ba, L, T), torch.zeros(Ba, L, T, dtype=torch.float64), A["w_t"], A["b_t"])
            aux = aux + m
            daux, taux = dm + U * aux.abs(), taux + tm
        if mode == "decoupled":
            y, dy, ty = _ln(aux, daux, A["aux_g"], A["aux_b"], 1e-5, 2 + 2 + 6)   # a lane's 4 (+ 4) values, the butterfly
            gt = A["gate"].double()
            aux, daux, taux = gt * y, gt.abs() * dy + U * (gt * y).abs(), gt.abs() * ty
        t = aux + A["b_v"].double()
        dt, terms = daux + U * t.abs(), taux + A["b_v"].double().abs()
    if qc is not None:
        R = qc.shape[1]
        sc = float(A["scale"])
        basis = A["basisc"].double()
        ctx = sc * torch.einsum("lr,brd->bld", basis, qc.double())
        tctx = abs(sc) * torch.einsum("lr,brd->bld", basis.abs(), qc.double().abs())
        t = t + ctx
        dt, terms = dt + (R + 1) * U * tctx + U * t.abs(), terms + tctx
    if qb is not None:
        t = t + qb.double()[:, None, :]
        dt, terms = dt + U * t.abs(), terms + qb.double().abs()[:, None, :]
    return t, dt, terms


def _add_params(g, L, D, T, R):
    rn = lambda *s, sc=1.0: sc * torch.randn(*s, generator=g)
    A = dict(pos=rn(L, D), b_v=rn(D, sc=0.3), aux_g=1 + rn(D, sc=0.2), aux_b=rn(D, sc=0.2), gate=0.1 + rn(D, sc=0.03),
             basisc=rn(L, R, sc=L ** -0.5), scale=torch.tensor([0.05]))
    if T:
        A.update(w_t=rn(D, T, sc=T ** -0.5), b_t=rn(D, sc=0.3))
    return A


@pytest.mark.parametrize("mode", ["none", "decoupled"])
@pytest.mark.parametrize("D", [16, 64, 132, 512])
def test_embed_add_against_fp64(D, mode, ftn, dev):
    B, R = 3, 4
    g = torch.Generator().manual_seed(D)
    for L in (1, 28, 97):
        for T in (0, 1, 5):
            A = _add_params(g, L, D, T, R)
            Ad = {k: v.to(dev) for k, v in A.items()}
            for dense, Bq, (epi, use_c, use_b) in [(False, 1, (1, 1, 1)), (True, 1, (1, 1, 1)), (False, B, (1, 1, 1)),
                                                   (True, B, (1, 1, 1)), (True, 1, (1, 0, 0)), (False, B, (0, 1, 1)),
                                                   (True, B, (1, 0, 1)), (False, 1, (0, 1, 0)), (False, B, (1, 1, 0))]:
                mark = None
                if T and epi:
                    mark = torch.randn(B if dense else 1, L, T, generator=g)
                qc = torch.randn(Bq, R, D, generator=g) if use_c else None
                qb = torch.randn(Bq, D, generator=g) if use_b else None
                ref, budget, terms = _add_ref(A, L, D, T, mode, mark, epi, qc, qb)
                kw = {}
                if epi:
                    kw.update(pos=Ad["pos"], b_v=Ad["b_v"])
                    if mark is not None:                           # batch stride 0 (the pipeline's .expand) or dense
                        kw.update(mark=mark.to(dev) if dense else mark.to(dev).expand(B, -1, -1),
                                  time=(Ad["w_t"], Ad["b_t"]))
                    if mode == "decoupled":
                        kw.update(aux=(Ad["aux_g"], Ad["aux_b"], 1e-5, Ad["gate"]))
                if qc is not None:
                    kw.update(q_coeff=qc.to(dev), basisc=Ad["basisc"], scale=Ad["scale"])
                if qb is not None:
                    kw.update(q_bias=qb.to(dev))
                buf, out = _guarded(dev, *ref.shape)                # Ba = 1 unless a dense mark or the terms have B rows
                got = ftn.runtime.embed_add(L, D, dev, out=out, **kw)
                torch.cuda.synchronize()
                assert _guards_intact(buf) and got.shape == ref.shape
                assert ref.shape[0] == (B if (dense and mark is not None) or (Bq > 1 and (use_c or use_b)) else 1)
                _measure(f"k_embed_add {mode}", got, ref, budget, terms)


@pytest.mark.parametrize("D", [64, 132])
def test_embed_add_layer_mode_and_misaligned_operands(D, ftn, dev):
    """"layer" mode: ``add`` is the "none" composition and the LayerNorm is the embedding kernel's; against the fp64
    embedding at that kernel's tolerance after its epilogue (rtol 2e-5 / atol 2e-5).  And the 4-byte-load form
    (operands one float off a boundary) has the bits of the 16-byte one."""
    g = torch.Generator().manual_seed(3 * D)
    B, L, N, T, R = 3, 28, 5, 5, 4
    A = _add_params(g, L, D, T, R)
    mark, qc, qb = torch.randn(B, L, T, generator=g), torch.randn(B, R, D, generator=g), torch.randn(B, D, generator=g)
    run = lambda put: ftn.runtime.embed_add(L, D, dev, pos=put(A["pos"]), b_v=put(A["b_v"]), mark=mark.to(dev),
                                            time=(put(A["w_t"]), put(A["b_t"])), q_coeff=put(qc), basisc=put(A["basisc"]),
                                            scale=A["scale"].to(dev), q_bias=put(qb))
    add = run(lambda t: t.to(dev))
    assert torch.equal(add, run(lambda t: _off1(t, dev)))
    ref, budget, terms = _add_ref(A, L, D, T, "layer", mark, 1, qc, qb)
    _measure("k_embed_add none", add, ref, budget, terms)
    x, w = torch.rand(B, L, N, generator=g) + 1.0, torch.randn(D, N, generator=g) / N ** 0.5
    gam, bet = 1 + 0.2 * torch.randn(D, generator=g), 0.2 * torch.randn(D, generator=g)
    got = ftn.runtime.embed_forward(x.to(dev), w.to(dev), add, (gam.to(dev), bet.to(dev), 1e-5))
    want = torch.nn.functional.layer_norm(x.double() @ w.double().T + ref, (D,), gam.double(), bet.double(), 1e-5)
    np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), rtol=2e-5, atol=2e-5)


# ------------------------------------------------------------------------------------------------------ whole model
def test_pipeline_fixture_on_the_device(ftn, dev):
    """``tests/golden/pipeline_predict_once.npz`` through the steps of ``test_predict_pipeline_dropin.py``, on the
    device: one series per batch row, per-sample statics and ids (Bc = B), every shell stage in HIP."""
    with np.load(GOLDEN / "pipeline_predict_once.npz") as f:
        z = {k: f[k] for k in f.files}
    ctor = json.loads(str(z["ctor_json"]))
    assert {k: ctor[k] for k in PIPE_MODEL} == json.loads(json.dumps(PIPE_MODEL))
    state = _part(z, "sd:")
    x, kw = torch.from_numpy(z["x"]).to(dev), {k: v.to(dev) for k, v in _part(z, "kw:").items()}
    model = ftn.models.TimesNet(**ctor)
    with torch.no_grad():
        model(torch.from_numpy(z["warm_x"]).to(dev), **{k: v.to(dev) for k, v in _part(z, "warm_kw:").items()})
    emb = state["series_embedding.weight"]
    if tuple(model.series_embedding.weight.shape) != tuple(emb.shape):
        model.series_embedding = torch.nn.Embedding(*emb.shape, dtype=emb.dtype)
    model.load_state_dict(state, strict=True)
    model.eval().to(dev)
    model._series_id_vocab = int(model.series_embedding.num_embeddings)
    model._series_id_reference = torch.arange(model._series_id_vocab, dtype=torch.long, device=dev)
    model._last_context_backend = model._last_embed_backend = model._last_head_backend = "unset"
    with torch.inference_mode():
        rate, disp = model(x, **kw)
    assert (model._last_context_backend, model._last_embed_backend, model._last_head_backend) == ("hip", "hip", "hip")
    assert kw["series_static"].ndim == 3 and kw["series_static"].size(0) == x.size(0) > 100      # Bc = B
    err = lambda a, b: float((np.abs(a.cpu().numpy() - b) / (ATOL + RTOL * np.abs(b))).max())
    print(f"PIPELINE_ERR rate {err(rate, z['rate']):.3f} disp {err(disp, z['disp']):.3f} of tol")
    np.testing.assert_allclose(rate.cpu().numpy(), z["rate"], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(disp.cpu().numpy(), z["disp"], rtol=RTOL, atol=ATOL)


def _ctx_mirrors(ftn, dev, mode, d_model, norm=None, N=24, L=24, H=6, T=3, seed=0):
    """``test_gpu_timeproj._mirrors`` with the whole context front end switched on: statics, ids, rank-4 temporal
    context, constant bias, late head, and time features."""
    cfg = dict(input_len=L, pred_len=H, d_model=d_model, d_ff=2 * d_model, n_layers=2, k_periods=3,
               kernel_set=[(3, 3), (5, 5)], dropout=0.0, activation="gelu", mode=mode, use_checkpoint=False,
               id_embed_dim=4, use_zero_mean_context=True, context_rank=4, use_constant_context_bias=True,
               use_late_bias_head=True)
    if norm is not None:
        cfg["embed_norm_mode"] = norm
    g = torch.Generator().manual_seed(seed + 1)
    kw = {"series_ids": torch.arange(N), "series_static": torch.randn(N, 3, generator=g)}
    torch.manual_seed(seed)
    cpu = ftn.models.TimesNet(**cfg).eval()
    with torch.no_grad():
        cpu(torch.rand(2, L, N, generator=g) + 1.0, torch.randn(2, L, T, generator=g), **kw)
        for p in cpu.parameters():                              # wake the zero-initialised heads / context maps
            if float(p.abs().sum()) == 0.0:
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
    gpu = ftn.models.TimesNet(**cfg).eval()
    dkw = {k: v.to(dev) for k, v in kw.items()}
    with torch.no_grad():
        gpu(torch.ones(2, L, N, device=dev), torch.zeros(2, L, T, device=dev), **dkw)
    gpu.load_state_dict(cpu.state_dict(), strict=True)
    t = torch.arange(L, dtype=torch.float32).view(1, L, 1)
    x = torch.rand(5, L, N, generator=g) + 1.5 + torch.sin(2 * torch.pi * t / 6.0)
    return cpu, gpu, x, torch.randn(5, L, T, generator=g), torch.randn(5, 12, T, generator=g), kw, dkw


@pytest.mark.parametrize("d_model", [64, 192])
@pytest.mark.parametrize("mode", ["direct", "recursive"])
def test_model_with_context_and_marks_matches_its_cpu_mirror(mode, d_model, ftn, dev):
    cpu, gpu, x, mark, _, kw, dkw = _ctx_mirrors(ftn, dev, mode, d_model)
    assert cpu.context_proj is not None and cpu.late_bias_head is not None and cpu.context_coeff.out_features == 4
    with torch.no_grad():
        want_r, want_d = cpu(x, mark, **kw)
    assert cpu._last_context_backend == "torch"
    with torch.inference_mode():
        rate, disp = gpu(x.to(dev), mark.to(dev), **dkw)
    assert (gpu._last_context_backend, gpu._last_embed_backend, gpu._last_head_backend) == ("hip", "hip", "hip")
    err = lambda a, b: float(((a.cpu() - b).abs() / (ATOL + RTOL * b.abs())).max())
    print(f"MODEL_ERR {mode} d_model={d_model}: rate {err(rate, want_r):.3f} disp {err(disp, want_d):.3f} of tol")
    np.testing.assert_allclose(rate.cpu().numpy(), want_r.numpy(), rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(disp.cpu().numpy(), want_d.numpy(), rtol=RTOL, atol=ATOL)


def test_graph_replay_is_bit_equal_to_eager(ftn, dev):
    _, gpu, x, mark, _, _, dkw = _ctx_mirrors(ftn, dev, "direct", 192)
    x, mark = x.to(dev), mark.to(dev)
    x2, mark2 = x.flip(0) * 1.25, mark.flip(0)
    with torch.inference_mode():
        want = [t.clone() for t in gpu(x, mark, **dkw)]
        want2 = [t.clone() for t in gpu(x2, mark2, **dkw)]
    gpu._last_context_backend = "unset"
    gf = ftn.graph.GraphedForward(gpu, x, mark, **dkw)
    got = [t.clone() for t in gf(x, mark, **dkw)]
    got2 = [t.clone() for t in gf(x2, mark2, **dkw)]
    torch.cuda.synchronize()
    assert gpu._last_context_backend == "hip"
    assert all(torch.equal(a, b) for a, b in zip(got, want)) and all(torch.equal(a, b) for a, b in zip(got2, want2))
    assert not torch.equal(want[0], want2[0])


@pytest.mark.parametrize("norm", ["none", "decoupled", "layer"])
def test_recursive_forecasts_with_marks_are_bit_equal_to_the_loop(norm, ftn, dev, monkeypatch):
    """The device recursion (one rows launch, ``add`` rebuilt per step from the step's marks) against the host loop,
    which calls the whole model at every step."""
    F, rt = ftn.forecast, ftn.runtime
    _, gpu, x, mark, y_mark, _, dkw = _ctx_mirrors(ftn, dev, "recursive", 64, norm=norm)
    assert gpu.embedding.embed_norm_mode == norm
    x, mark, y_mark, H = x.to(dev), mark.to(dev), y_mark.to(dev), 9
    calls = {"rows": 0, "add": 0}
    rows_fn, add_fn = rt.context_rows, rt.embed_add
    monkeypatch.setattr(rt, "context_rows", lambda *a, **k: (calls.__setitem__("rows", calls["rows"] + 1), rows_fn(*a, **k))[1])
    monkeypatch.setattr(rt, "embed_add", lambda *a, **k: (calls.__setitem__("add", calls["add"] + 1), add_fn(*a, **k))[1])
    with torch.inference_mode():
        assert F._device_ok(gpu, x, H, mark, y_mark, dkw["series_static"], dkw["series_ids"])
        want_r, want_d = F.forecast_recursive_batch_loop(gpu, x, H, mark, y_mark, **dkw)
        assert (calls["rows"], calls["add"]) == (H, H)
        got_r, got_d = F.forecast_recursive_batch(gpu, x, H, mark, y_mark, **dkw)
        assert (calls["rows"], calls["add"]) == (H + 1, 2 * H)                 # the device path: one rows launch
    torch.cuda.synchronize()
    assert gpu._last_context_backend == "hip" and got_r.shape == (5, H, 24)
    assert torch.equal(got_r, want_r) and torch.equal(got_d, want_d)


# ---------------------------------------------------------------------------------------------------- what ran (last)
def test_every_context_kernel_was_measured():
    assert {"rows", "coeff", "cbias", "late", "k_through_small", "k_through_chunks", "k_embed_add none",
            "k_embed_add decoupled"} <= set(E_MAX)
    for name, (e, cap) in sorted(E_MAX.items()):
        print(f"CONTEXT_E {name:22s} max e = {e:6.2f} u   cap of that element = {cap:7.2f} u")
