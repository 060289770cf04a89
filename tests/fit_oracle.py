"""What tests/test_fit_host.py and tests/test_gpu_fit.py measure ``fit.nb_nll_grad`` against: the lattice, two
independent oracles of the log-likelihood's derivatives in 40-digit arithmetic (mpmath, which torch's own dependency
sympy brings), and the bound.  Each oracle is computed once per process and never changed.

Oracle 1 differentiates the restated formula itself (``mpmath.diff`` of losses.py:47-53, nothing derived by hand).
fp64 autograd of the same formula is NOT accurate enough to be an oracle here: ``digamma(y + r) - digamma(r)`` loses
``psi(r) 2^-52 / alpha^2``, measured on the lattice at up to 6.8 times the bound below, so the differentiation runs in
40 digits.  Oracle 2 is the closed form with ``psi(y + r) - psi(r) = sum_{j < y} 1 / (r + j)`` for the integer ``y``.

The bound: ``|err| <= 4 2^-24 |g| + 2^-36 (log1p(alpha mu) + dpsi) / alpha^2`` - the final rounding to fp32 with
room for the scale multiply, and the accuracy class ``ftn_nbmath.h`` documents for its series (6e-12) amplified by the
formula's own ``1 / alpha^2``.
"""
import functools

import mpmath as mp
import numpy as np
import torch

ALPHAS = (1e-3, 3e-3, 1e-2, 0.1, 1.0, 30.0)
LOG_MUS = tuple(range(-6, 7))
YS = (0.0, 1.0, 2.0, 7.0, 50.0, 400.0, 0.37, 12.5)
DPS = 40


def lattice():
    """``(y, rate, disp)`` fp32 [6, 13, 8]: every combination."""
    al = torch.tensor(ALPHAS, dtype=torch.float32)
    mu = torch.exp(torch.tensor(LOG_MUS, dtype=torch.float64)).float()
    yy = torch.tensor(YS, dtype=torch.float32)
    A, M, Y = torch.meshgrid(al, mu, yy, indexing="ij")
    return Y.contiguous(), M.contiguous(), A.contiguous()


def _ll(y, mu, al):
    """losses.py:47-53, restated."""
    r = 1 / al
    l1 = mp.log1p(al * mu)
    return (mp.loggamma(y + r) - mp.loggamma(r) - mp.loggamma(y + 1) - r * l1 + y * (mp.log(al) + mp.log(mu) - l1))


def _each(y, rate, disp):
    for yv, mv, av in zip(y.reshape(-1).tolist(), rate.reshape(-1).tolist(), disp.reshape(-1).tolist()):
        yield mp.mpf(max(yv, 0.0)), mp.mpf(mv), mp.mpf(av)      # the fp32 values, exactly


def by_differentiation(y, rate, disp):
    """Oracle 1: ``(d ll / d rate, d ll / d dispersion)`` fp64 arrays, of finite fp32 tensors above ``eps``."""
    with mp.workdps(DPS):
        out = [(mp.diff(lambda m: _ll(yv, m, av), mv), mp.diff(lambda a: _ll(yv, mv, a), av))
               for yv, mv, av in _each(y, rate, disp)]
    g = np.array([[float(a), float(b)] for a, b in out]).reshape(tuple(y.shape) + (2,))
    return g[..., 0], g[..., 1]


def closed_form(y, rate, disp, finite_sum=False):
    """``(g_rate, g_disp, ll, amp)`` fp64 arrays from the closed forms; ``amp = (log1p(alpha mu) + dpsi) / alpha^2`` is
    what the bound's second term scales.  ``finite_sum`` (oracle 2): ``dpsi`` as ``sum_{j < y} 1 / (r + j)``, NaN
    where ``y`` is not an integer; otherwise two 40-digit digammas."""
    rows = []
    with mp.workdps(DPS):
        for yv, mv, av in _each(y, rate, disp):
            r, t = 1 / av, av * mv
            l1 = mp.log1p(t)
            if not finite_sum:
                dpsi = mp.digamma(yv + r) - mp.digamma(r)
            elif yv == int(yv):
                dpsi = mp.fsum(1 / (r + j) for j in range(int(yv)))
            else:
                dpsi = mp.nan
            rows.append(((yv - mv) / (mv * (1 + t)), (l1 - dpsi) / av ** 2 + (yv - mv) / (av * (1 + t)),
                         _ll(yv, mv, av), (l1 + dpsi) / av ** 2))
    g = np.array([[float(v) for v in row] for row in rows]).reshape(tuple(y.shape) + (4,))
    return g[..., 0], g[..., 1], g[..., 2], g[..., 3]


def bound(g, amp=None):
    """The bound on a raw derivative ``g`` (fp64 array); ``amp`` only for the dispersion's.  1e-45 is room for
    oracle 1 itself: where ``y == mu`` the rate's derivative is exactly 0 and the 40-digit differentiation returns
    4e-50 (measured).  It is below the smallest positive fp32, so no error of an fp32 result fits under it."""
    b = 4 * 2.0 ** -24 * np.abs(g) + 1e-45
    return b if amp is None else b + 2.0 ** -36 * amp


@functools.lru_cache(maxsize=None)
def lattice_oracles():
    """``(oracle 1, oracle 2, closed form in 40 digits)`` on the lattice."""
    y, rate, disp = lattice()
    return by_differentiation(y, rate, disp), closed_form(y, rate, disp, finite_sum=True), closed_form(y, rate, disp)


def valid_of(y, rate, disp, mask=None, eps=1e-8):
    """The reference's validity (losses.py:36-55) as a bool array, and the operands with every invalid element
    replaced by a harmless one (so the oracles can run over the whole array)."""
    yc = torch.clamp(y, min=0.0)
    e = torch.tensor(eps, dtype=torch.float32)
    mu, al = torch.maximum(rate, e), torch.maximum(disp, e)
    valid = torch.isfinite(yc) & torch.isfinite(mu) & torch.isfinite(al)
    if mask is not None:
        valid = valid & mask.to(torch.bool)
    one = torch.ones(())
    return valid, torch.where(valid, yc, 0 * one), torch.where(valid, mu, one), torch.where(valid, al, one)
