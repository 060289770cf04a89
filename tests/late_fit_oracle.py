"""The fp64 side of the late-bias refit tests (tests/test_late_fit_host.py, tests/test_late_forms_table.py,
tests/test_gpu_late_fit.py): the torch composition ``gate * linear(layer_norm(rows))^T`` in fp64 under autograd, the
shape grid, the inputs and the a-priori error bounds of the five gradients ``ftn_late_backward`` returns.

Parameter order everywhere: ``(gamma, beta, weight, bias, gate)``, the argument order of ``fit.late_bias``.

The bounds.  U = 2^-24; every bound is (roundings along the gradient's chain) * U * (the fp64 sum of the absolute
values of the products along that chain), first order in U.  For one row r with c its ``ctx`` values, m their mean,
v = c - m, xh = v rstd, z = xh gamma + beta, u = W z + b, Gs = sum_b d_pre, du = gate Gs, dz = du^T W:

* the mean is a sum of ctx values and a division: at most ctx + 8 roundings (the lane's slots, six butterfly steps, the
  division) against mean|c|; the subtraction adds one: |dv_k| <= U (|v_k| + (ctx + 8) mean|c|), that is a relative
  error rho_k = 1 + (ctx + 8) mean|c| / |v_k| - which is why a purely relative bound needs |v_k| away from 0: the
  inputs below have |xh| >= 1e-3 (asserted; rows that miss 0.05 are drawn again), and rho = max_k rho_k is taken per
  row from the data.  rstd carries the variance's 2 rho + ctx + 8 halved, and the eps addition, the root and the
  division: rho + (ctx + 8) / 2 + 3.  So xh_k is off by at most ex_k = Ex |xh_k| (in units of U) with
  Ex = 2 rho + (ctx + 8) / 2 + 4.
  ctx == 1 is the one size where no relative bound exists: v = c - c / 1 is 0 in exact arithmetic, so xh = 0, while an
  implementation whose mean is off by a few ulps of |c| (torch's is, in fp32 and in fp64) has v != 0 and multiplies it
  by rstd = 1 / sqrt(eps).  There the absolute form of the same count is used: ex = (ctx + 8) |c| rstd.
* z_k: the fmaf rounds once: ez_k = ex_k |gamma_k| + Za_k with Za = |xh gamma| + |beta|.
* u_s: a chain of ctx fmaf and the bias: eu_s = (ctx + 2) Ua_s + sum_k |W_sk| ez_k with Ua = |W| Za + |b|.
* Gs: B - 1 additions (none for Bc == B); du: one product.  With Ga = sum_b |d_pre|: |d du| <= U B |gate| Ga.
* a sum over R rows passes at most R + 2 additions (a chain over the chunk's rows, then the chunks in order);
  base = R + 2 + B counts them with Gs' and du's.
* dz_k = sum_s du_s W_sk: S fmaf, against DZa_k with DZa = (|gate| Ga) |W|.

  dgate[s]  = sum_r Gs u         U  sum_r Ga ((base + 1) Ua + eu)
  db[s]     = sum_r du           U  base sum_r |gate| Ga
  dW[s][k]  = sum_r du z         U  sum_r |gate| Ga ((base + 1) Za + ez)
  dbeta[k]  = sum_r dz           U  (base + S) sum_r DZa
  dgamma[k] = sum_r dz xh        U  sum_r DZa ((base + S + 1) |xh| + ex)

The fp64 reference's own error has the same structure with 2^-53 for U: 2^-29 of the bound.  torch's fp32 autograd of
the composition on the same inputs lies inside these bounds over the whole grid (tests/test_late_fit_host.py checks it
on the CPU)."""
import functools

import torch

U = 2.0 ** -24
NAMES = ("late_bias_norm.weight", "late_bias_norm.bias", "late_bias_head.weight", "late_bias_head.bias",
         "late_bias_gate")
EPS = 1e-5
CHUNK = 256                                                     # series rows of a chunk (LF_CHUNK)
CTXS = [1, 3, 63, 64, 65, 130, 256]
SS = [1, 4, 63, 64, 65, 97]
RS = [1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3]
# how the R rows lie: ("wide", B): Bc = 1, N = R, d_pre [B, S, R]; ("pipe", 1): Bc = B = R, N = 1; ("pipe", 0): Bc = B
# the smallest factor of R above 1 (R itself when it has none), N = R / Bc
LAYOUTS = [("wide", 1), ("wide", 2), ("wide", 5), ("pipe", 1), ("pipe", 0)]
# every ctx, S, R and layout appears, rotated against each other
GRID = [(CTXS[i % 7], SS[(i + i // 7) % 6], RS[(i + i // 6) % 5], LAYOUTS[(2 * i + i // 5) % 5]) for i in range(35)]
FORMS = {"k_late_bwd_mfma"}                                     # the forms csrc/latefit.hip defines


def dims(R, layout):
    """``(B, Bc, N)`` of ``R`` rows in ``layout``."""
    kind, arg = layout
    if kind == "wide":
        return arg, 1, R
    if arg == 1:
        return R, R, 1
    Bc = next((f for f in range(2, R + 1) if R % f == 0), 1)
    return Bc, Bc, R // Bc


@functools.lru_cache(maxsize=None)
def case(i):
    """``(rows [Bc, N, ctx], params, d_pre [B, S, N])`` of grid entry i, fp32 on the CPU.  Rows: +-(0.5 .. 1.5) with
    random signs, so the centred values are of order 1; the oracle asserts ``min |xh| >= 1e-3`` (ctx > 1)."""
    ctx, S, R, layout = GRID[i]
    B, Bc, N = dims(R, layout)
    g = torch.Generator().manual_seed(9100 + i)
    rnd = lambda *shape: torch.randn(*shape, generator=g)
    sign = torch.where(torch.rand(Bc, N, ctx, generator=g) < 0.5, -1.0, 1.0)
    rows = (sign * (0.5 + torch.rand(Bc, N, ctx, generator=g))).float()
    for _ in range(64 if ctx > 1 else 0):                       # rows with a centred value near 0 are drawn again
        v = rows.double() - rows.double().mean(-1, keepdim=True)
        near = ((v.abs() / torch.sqrt((v * v).mean(-1, keepdim=True) + EPS)).min(-1).values < 0.05)
        if not bool(near.any()):
            break
        fresh = torch.randn(Bc, N, ctx, generator=g).float()
        rows = torch.where(near.unsqueeze(-1), fresh, rows)
    params = (1.0 + 0.3 * rnd(ctx), 0.3 * rnd(ctx), rnd(S, ctx) / max(ctx, 1) ** 0.5, 0.3 * rnd(S),
              (0.05 + 0.05 * rnd(S)).reshape(1, S, 1))
    d_pre = (rnd(B, S, N) / (B * S * N)).float()
    return rows, tuple(p.float() for p in params), d_pre


def late64(rows, p64):
    """The composition in the dtype of ``p64``: ``[Bc, S, N]``."""
    gamma, beta, weight, bias, gate = p64
    lb = torch.nn.functional.linear(
        torch.nn.functional.layer_norm(rows.to(gamma.dtype), (rows.shape[-1],), gamma, beta, EPS), weight, bias)
    return gate.reshape(1, -1, 1) * lb.transpose(1, 2)


def grads_of(rows, params, d_pre, dtype=torch.float64):
    """The five gradients of ``sum(late * d_pre)`` (``late`` broadcast over the batch) by autograd in ``dtype``."""
    p = [t.detach().to(dtype).requires_grad_() for t in params]
    late = late64(rows, p)
    return torch.autograd.grad((late * d_pre.to(dtype)).sum(), p)


def grads_and_bounds(rows, params, d_pre, extra=0):
    """``(gradients, bounds)`` in fp64, in the parameter order above (the gate's as ``[1, S, 1]``).  ``extra``: the
    roundings ``d_pre`` itself carries when it is not an input but the output of a forward and a loss gradient (the
    end-to-end tests); it joins ``base``, which every product of every chain is charged with."""
    want = [w.detach() for w in grads_of(rows, params, d_pre)]
    gamma, beta, weight, bias, gate = (t.detach().double() for t in params)
    Bc, N, ctx = rows.shape
    B, S = d_pre.shape[:2]
    R = Bc * N
    c = rows.double().reshape(R, ctx)
    mean = c.mean(1, keepdim=True)
    v = c - mean
    xh = v / torch.sqrt((v * v).mean(1, keepdim=True) + EPS)
    if ctx > 1:
        assert float(xh.abs().min()) >= 1e-3, "a centred value too close to 0 for a relative bound"
        rho = 1 + (ctx + 8) * c.abs().mean(1, keepdim=True) / v.abs().min(1, keepdim=True).values
        ex = (2 * rho + (ctx + 8) / 2 + 4) * xh.abs()             # [R, ctx]
    else:
        ex = (ctx + 8) * c.abs() / EPS ** 0.5
    Za = (xh * gamma).abs() + beta.abs()                          # [R, ctx]
    ez = ex * gamma.abs() + Za
    Ua = Za @ weight.abs().T + bias.abs()                         # [R, S]
    eu = (ctx + 2) * Ua + ez @ weight.abs().T
    dp = d_pre.double().abs()
    Ga = (dp.sum(0, keepdim=True) if Bc == 1 else dp).permute(0, 2, 1).reshape(R, S)
    Bsum = B if Bc == 1 else 1
    dua = gate.reshape(1, S).abs() * Ga                           # [R, S]
    DZa = dua @ weight.abs()                                      # [R, ctx]
    base = R + 2 + Bsum + extra
    bounds = [U * (DZa * ((base + S + 1) * xh.abs() + ex)).sum(0),
              U * (base + S) * DZa.sum(0),
              U * torch.einsum("rs,rk->sk", dua, (base + 1) * Za + ez),
              U * base * dua.sum(0),
              (U * (Ga * ((base + 1) * Ua + eu)).sum(0)).reshape(1, S, 1)]
    return want, bounds


def fraction(got, want, bounds):
    """The largest ``|got - want| / bound`` over the five tensors (a zero bound takes a zero error)."""
    worst = 0.0
    for a, b, bd in zip(got, want, bounds):
        err = (a.detach().double().cpu().reshape(b.shape) - b.cpu()).abs()
        bd = bd.cpu().reshape(b.shape)
        assert bool((err[bd == 0] == 0).all()), "an error where the bound is exactly 0"
        worst = max(worst, float((err / bd.clamp_min(1e-300)).max()))
    return worst


def lattice_case(R, S=5):
    """The exactness case: ``(rows, params, d_pre, want)`` with every intermediate an integer that fp32 holds
    exactly.  Rows are ``(+a, -a, 0, 0, 0, 0, 0, 0)`` with ``a = 2^j``, signs drawn per row: the mean is exactly 0 in
    any summation order, the variance 2 a^2 / 8 = a^2 / 4, and with eps = 0 (which the test passes) rstd = 2 / a, so
    xh = (+-2, -+2, 0, ...) exactly - asserted here in fp32.  gamma = 1, beta = 0, so z = xh; W, b, gate and d_pre are
    small integers.  ``want``: the five gradients of the integer lattice, computed in int64 (Bc == B, N = 1)."""
    g = torch.Generator().manual_seed(77 + R)
    ctx = 8
    a = 2.0 ** torch.randint(-3, 4, (R, 1), generator=g).float()
    sign = torch.where(torch.rand(R, 1, generator=g) < 0.5, -1.0, 1.0)
    rows = torch.cat([sign * a, -sign * a, torch.zeros(R, ctx - 2)], dim=1).float()
    xh = torch.cat([2 * sign, -2 * sign, torch.zeros(R, ctx - 2)], dim=1)
    got = torch.nn.functional.layer_norm(rows, (ctx,), None, None, 0.0)
    assert torch.equal(got, xh), "the lattice rows do not normalise exactly"
    xh = xh.long()
    W = torch.randint(-3, 4, (S, ctx), generator=g)
    b = torch.randint(-3, 4, (S,), generator=g)
    gate = torch.randint(-2, 3, (S,), generator=g)
    dp = torch.randint(-4, 5, (R, S), generator=g)               # d_pre[b, s, 0]
    u = xh @ W.T + b
    du = gate * dp
    want = {"dgate": (dp * u).sum(0), "db": du.sum(0), "dW": du.T @ xh, "dbeta": (du @ W).sum(0),
            "dgamma": ((du @ W) * xh).sum(0)}
    params = (torch.ones(ctx), torch.zeros(ctx), W.float(), b.float(), gate.float().reshape(1, S, 1))
    return rows.reshape(R, 1, ctx), params, dp.float().reshape(R, S, 1), want
