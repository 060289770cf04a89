"""The negative binomial of a forecast in torch ops, on any device: the reference the ``hip`` kernels of
csrc/quantile.hip and csrc/sample.hip are held to, and what ``score`` runs where they cannot.  Pure functions: no
backend choice is made here.

``F(y) = I_p(r, floor(yc) + 1)``, ``r = 1 / alpha``, ``p = 1 / (1 + alpha mu)`` with the scorer's clamps; ``Q(q)`` the
smallest integer k >= 0 with ``F(k) >= q``.  ``_nb_cdf_torch`` is k_nb_cdf, ``_nb_search`` is ``nq_level``
(csrc/ftn_nbq.h): the same continued fraction and the same bracketed search in fp64.  ``_nb_quantiles_torch`` walks
the levels in ascending order around it as k_nb_quantile does, ``_nb_invert_torch`` starts it as k_nb_sample does.

Draw s of element e is ``Q(u(e, s))``: one uniform per draw, so a draw is a pure function of (seed, offset, e, s), the
same on any device, grid, kernel form and backend.  The uniforms (``sample_uniforms``):
  Philox4x32-10, key = (seed & 0xffffffff, seed >> 32), counter = (e & 0xffffffff, e >> 32, s >> 2, offset),
  e the row-major index of the element in ``shape``; draw s takes output word s & 3; u = (word + 0.5) 2^-32 (fp64).
"""
from __future__ import annotations

from statistics import NormalDist

import torch

NBQ_QMAX = 8                 # levels of one k_nb_quantile launch (FTN_QMAX)
NBQ_KLIM = float(1 << 24)    # answers below it are exact in fp32; at or beyond it: NaN and flag bit 1
NBQ_FLAG_RANGE = 2           # bit 1 of the flag word
_NBQ_CF_MAX = 4096           # continued-fraction iterations (the kernel's NBQ_CF_MAX)
_NBQ_EVALS = 32              # CDF evaluations of one level: 6 Newton steps, then 25 halvings of [0, 2^24] and one spare
_NBQ_NEWTON = 6
_NBQ_WALK = 64               # pmf-recurrence steps after an evaluation


def _nbq_params(rate, dispersion, eps):
    """``(r, t, p, 1 - p, log p, log(1 - p), valid)`` in fp64 from fp32-rounded inputs, the scorer's clamps."""
    al = dispersion.to(torch.float32)
    mu = rate.to(torch.float32)
    e = torch.tensor(eps, dtype=torch.float32, device=al.device)
    al = torch.where(al < e, e, al)
    mu = torch.where(mu < e, e, mu)
    valid = torch.isfinite(al) & torch.isfinite(mu)
    one = torch.ones_like(al)
    al, mu = torch.where(valid, al, one).double(), torch.where(valid, mu, one).double()
    r, t = 1.0 / al, al * mu
    return r, t, 1.0 / (1.0 + t), t / (1.0 + t), -torch.log1p(t), -torch.log1p(1.0 / t), valid


def _stirling_corr(x):
    z = 1.0 / x
    z2 = z * z
    return z * (1.0 / 12.0 + z2 * (-1.0 / 360.0 + z2 * (1.0 / 1260.0 + z2 * (-1.0 / 1680.0))))


def _log_inv_beta(a, b):
    """lgamma(a + b) - lgamma(a) - lgamma(b); for max(a, b) >= 16 the two large lgammas are differenced in
    Stirling's form, which keeps 1e8-sized terms from cancelling."""
    L, S = torch.maximum(a, b), torch.minimum(a, b)
    big = L >= 16.0
    Ls = torch.where(big, L, torch.full_like(L, 16.0))
    ratio = S * torch.log(Ls + S) + (Ls - 0.5) * torch.log1p(S / Ls) - S + _stirling_corr(Ls + S) - _stirling_corr(Ls)
    return torch.where(big, ratio, torch.lgamma(L + S) - torch.lgamma(L)) - torch.lgamma(S)


def _betacf(a, b, x, iters=_NBQ_CF_MAX):
    """The continued fraction of I_x(a, b) by the modified Lentz method; ``(h, converged)``."""
    tiny = 1e-300
    qab, qap, qam = a + b, a + 1.0, a - 1.0
    c = torch.ones_like(a)
    d = 1.0 - qab * x / qap
    d = 1.0 / torch.where(d.abs() < tiny, torch.full_like(d, tiny), d)
    h = d.clone()
    live = torch.ones_like(a, dtype=torch.bool)
    for m in range(1, iters + 1):
        m2 = 2.0 * m
        aa = m * (b - m) * x / ((qam + m2) * (a + m2))
        d = 1.0 + aa * d
        d = 1.0 / torch.where(d.abs() < tiny, torch.full_like(d, tiny), d)
        c = 1.0 + aa / c
        c = torch.where(c.abs() < tiny, torch.full_like(c, tiny), c)
        h1 = h * d * c
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2))
        d = 1.0 + aa * d
        d = 1.0 / torch.where(d.abs() < tiny, torch.full_like(d, tiny), d)
        c = 1.0 + aa / c
        c = torch.where(c.abs() < tiny, torch.full_like(c, tiny), c)
        de = d * c
        h = torch.where(live, h1 * de, h)
        live = live & ~((de - 1.0).abs() < 1e-13)
        if m % 8 == 0 and not bool(live.any()):
            break
    return h, ~live


def _nb_cdf_pmf(k, r, p, omp, lp, lomp):
    """``(F(k), pmf(k), converged)`` for integer-valued fp64 k >= 0."""
    a, b = r, k + 1.0
    front = torch.exp(_log_inv_beta(a, b) + a * lp + b * lomp)
    swap = p * (a + b + 2.0) >= a + 1.0
    h, ok = _betacf(torch.where(swap, b, a), torch.where(swap, a, b), torch.where(swap, omp, p))
    F = torch.where(swap, 1.0 - front * h / b, front * h / a)
    return F.clamp(0.0, 1.0), front / ((k + r) * omp), ok


def _nb_cdf_torch(y, rate, dispersion, eps):
    r, t, p, omp, lp, lomp, valid = _nbq_params(rate, dispersion, eps)
    yf = y.to(torch.float32)
    yc = torch.where(yf < 0, torch.zeros_like(yf), yf)
    valid = valid & torch.isfinite(yc)
    k = torch.floor(torch.where(valid, yc, torch.zeros_like(yc)).double())
    inside = k < NBQ_KLIM
    F, _, ok = _nb_cdf_pmf(torch.where(inside, k, torch.zeros_like(k)), r, p, omp, lp, lomp)
    bad = valid & ~(inside & ok)
    F = torch.where(valid & ~bad, F, torch.full_like(F, float("nan")))
    return F, bad.any().to(torch.int32) * NBQ_FLAG_RANGE


def _nbq_guess(z, r, t, omp, p):
    """Cornish-Fisher start: mean + sd (z + skew (z^2 - 1) / 6), floored into [0, 2^24)."""
    mean = r * t
    sd = torch.sqrt(mean * (1.0 + t))
    skew = (2.0 - p) / torch.sqrt(r * omp)
    g = torch.floor(mean + sd * (z + skew * (z * z - 1.0) / 6.0))
    return torch.nan_to_num(g, nan=0.0, posinf=NBQ_KLIM - 1.0, neginf=0.0).clamp(0.0, NBQ_KLIM - 1.0)


def _nb_search(q, z, par, state):
    """``nq_level`` in torch ops: one level per element (``q`` a float or an fp64 tensor strictly inside (0, 1), ``z``
    its standard normal quantile, which only seeds the search), continuing from ``state = (k, F, pm, have, prev)``:
    the last point whose F(k) and pmf(k) are known where ``have``, and the answer to the level before.  ``par``:
    ``_nbq_params``.  The CDF is evaluated for the elements that still search only.  Returns ``(answer fp32, any valid
    element without one, the state to go on from)``; NaN where the element is not valid, the answer is >= 2^24 or a
    cap was reached."""
    r, t, p, omp, lp, lomp, valid = par
    k, F, pm, have, prev = state
    F, pm = F.clone(), pm.clone()
    g = torch.maximum(_nbq_guess(z, r, t, omp, p), prev)
    lo, hi = prev.clone(), torch.full_like(r, NBQ_KLIM)         # the answer lies in [lo, hi]
    need = ~(have & (g <= k + _NBQ_WALK))                       # near the last known point: walk on from it
    k = torch.where(need, g, k)
    done = ~valid
    for it in range(_NBQ_EVALS):
        m = need & ~done
        if bool(m.any()):
            Fe, pe, ok = _nb_cdf_pmf(k[m], r[m], p[m], omp[m], lp[m], lomp[m])
            F[m], pm[m] = Fe, pe
            done[m] = ~ok                                       # the fraction's cap: lo < hi stays, so NaN below
        for _ in range(_NBQ_WALK):
            act = ~done
            down = act & (F >= q) & (k > lo) & (F - pm >= q)
            up = act & (F < q) & (k + 1.0 < NBQ_KLIM)
            if not bool((down | up).any()):
                break
            Fd, pd = F - pm, pm * k / ((k - 1.0 + r) * omp)
            pu = pm * (k + r) / (k + 1.0) * omp
            F = torch.where(down, Fd, torch.where(up, F + pu, F))
            pm = torch.where(down, pd, torch.where(up, pu, pm))
            lo = torch.where(up, k + 1.0, lo)
            k = torch.where(down, k - 1.0, torch.where(up, k + 1.0, k))
        ge = F >= q
        hi = torch.where(~done & ge, torch.minimum(hi, k), hi)
        lo = torch.where(~done & ~ge, k + 1.0, lo)
        found = ~done & ge & ((k <= lo) | (F - pm < q))
        lo = torch.where(found, k, lo)
        hi = torch.where(found, k, hi)
        done = done | found | (lo >= hi)
        kn = torch.floor(k + (q - F) / pm + 0.5)
        newton = (it < _NBQ_NEWTON) & (kn >= lo) & (kn < hi)
        kn = torch.where(newton, kn, torch.floor(0.5 * (lo + hi)))
        need = ~done
        k = torch.where(need, kn.clamp(max=NBQ_KLIM - 1.0), k)
        if bool(done.all()):
            break
    ans_ok = valid & (lo >= hi) & (hi < NBQ_KLIM)
    out = torch.where(ans_ok, hi, torch.full_like(hi, float("nan"))).to(torch.float32)
    return out, (valid & ~ans_ok).any(), (k, F, pm, ans_ok & (k == hi), torch.where(ans_ok, hi, prev))


def _nb_quantiles_torch(rate, dispersion, levels, eps):
    """``(out fp32 [Q, *rate.shape], flag)``: the levels in ascending order, each element's search continuing from
    its answer to the level before (k_nb_quantile)."""
    par = _nbq_params(rate, dispersion, eps)
    zero = torch.zeros_like(par[0])
    state = (zero, zero, zero, torch.zeros_like(par[6]), zero)
    out = torch.empty((len(levels),) + tuple(rate.shape), dtype=torch.float32, device=rate.device)
    bad_any = torch.zeros((), dtype=torch.bool, device=rate.device)
    for i in sorted(range(len(levels)), key=lambda i: levels[i]):
        q = float(levels[i])
        out[i], bad, state = _nb_search(q, NormalDist().inv_cdf(q), par, state)
        bad_any = bad_any | bad
    return out, bad_any.to(torch.int32) * NBQ_FLAG_RANGE


def _nb_invert_torch(q, rate, dispersion, eps):
    """The smallest integer k >= 0 with F(k) >= q for a level per element: ``q`` fp64 ``[S, *rate.shape]`` strictly
    inside (0, 1).  The search with the kernel's start (k_nb_sample): from the known point (0, p^r, p^r) where p^r has
    not underflowed and the Cornish-Fisher guess is within the walk of 0, else from the guess.  ``(out fp32, flag)``."""
    shape = tuple(q.shape)
    par = tuple(v.expand(shape).reshape(-1) for v in _nbq_params(rate, dispersion, eps))
    q = q.reshape(-1)
    pm0 = torch.exp(par[0] * par[4])                            # pmf(0) = F(0) = p^r
    zero = torch.zeros_like(pm0)
    out, bad, _ = _nb_search(q, torch.special.ndtri(q), par, (zero, pm0, pm0, pm0 > 0.0, zero))
    return out.reshape(shape), bad.to(torch.int32) * NBQ_FLAG_RANGE


_M32 = 0xFFFFFFFF
_PHILOX_M = (0xD2511F53, 0xCD9E8D57)
_PHILOX_W = (0x9E3779B9, 0xBB67AE85)


def _mulhilo32(m: int, c: torch.Tensor):
    """``(high, low)`` 32-bit words of ``m * c`` for a 32-bit constant m and int64 c in [0, 2^32): by 16-bit halves of
    c, so nothing leaves int64."""
    a, b = m * (c & 0xFFFF), m * (c >> 16)                      # each below 2^48
    return (b + (a >> 16)) >> 16, (a + ((b & 0xFFFF) << 16)) & _M32


def philox4x32(counter, key):
    """Philox4x32-10 (Salmon et al., SC 2011) in int64 torch ops: ``counter`` four and ``key`` two 32-bit words, each
    an int or an int64 tensor (broadcast together); returns the four output words as int64 tensors in [0, 2^32)."""
    c = [w if isinstance(w, torch.Tensor) else torch.tensor(int(w) & _M32, dtype=torch.int64) for w in counter]
    dev = next((w.device for w in list(counter) + list(key) if isinstance(w, torch.Tensor)), torch.device("cpu"))
    c0, c1, c2, c3 = (w.to(device=dev, dtype=torch.int64) for w in c)
    k0, k1 = (w.to(device=dev, dtype=torch.int64) if isinstance(w, torch.Tensor) else int(w) & _M32 for w in key)
    for _ in range(10):
        h0, l0 = _mulhilo32(_PHILOX_M[0], c0)
        h1, l1 = _mulhilo32(_PHILOX_M[1], c2)
        c0, c1, c2, c3 = h1 ^ c1 ^ k0, l1, h0 ^ c3 ^ k1, l0
        k0, k1 = (k0 + _PHILOX_W[0]) & _M32, (k1 + _PHILOX_W[1]) & _M32
    return c0, c1, c2, c3


def _seed_key(seed, device):
    """The key words of ``seed``: a Python int (its low 64 bits) or a one-element int64 / uint64 tensor."""
    if isinstance(seed, torch.Tensor):
        if seed.numel() != 1 or seed.dtype not in (torch.int64, torch.uint64):
            raise ValueError("seed must be a Python int or a one-element int64 / uint64 tensor")
        w = seed.reshape(1).view(torch.int64).to(device)
        return w & _M32, (w >> 32) & _M32
    s = int(seed) & 0xFFFFFFFFFFFFFFFF
    return s & _M32, s >> 32


def sample_uniforms(n_samples: int, shape, seed=0, offset: int = 0, device=None) -> torch.Tensor:
    """The uniforms of ``nb_sample`` for elements of ``shape`` (row-major index e): fp64 ``[n_samples, *shape]``,
    ``u[s, e] = (word + 0.5) 2^-32`` with ``word`` output ``s & 3`` of Philox4x32-10 at counter
    ``(e & 0xffffffff, e >> 32, s >> 2, offset)`` and key ``(seed & 0xffffffff, seed >> 32)``.  Strictly inside
    (0, 1); draws ``s < S1`` of a longer call are those of the ``S1`` call."""
    S = int(n_samples)
    if S < 1:
        raise ValueError(f"sample_uniforms: n_samples={n_samples}")
    if not 0 <= int(offset) <= _M32:
        raise ValueError(f"sample_uniforms: offset={offset} is not a 32-bit word")
    shape = tuple(int(v) for v in shape)
    dev = torch.device(device) if device is not None else (seed.device if isinstance(seed, torch.Tensor)
                                                           else torch.device("cpu"))
    n = 1
    for v in shape:
        n *= v
    e = torch.arange(n, dtype=torch.int64, device=dev)
    key = _seed_key(seed, dev)
    words = []
    for blk in range((S + 3) // 4):
        words.extend(philox4x32((e & _M32, e >> 32, blk, int(offset)), key))
    w = torch.stack([t.expand(n) for t in words[:S]])
    return ((w.to(torch.float64) + 0.5) * 2.0 ** -32).reshape((S,) + shape)
