"""What the refit-step tests share: the fp64 restatement of ``ftn_refit_update``'s formulas (include/flowtimes.h) in
numpy, torch's own ``clip_grad_norm_`` + ``AdamW(foreach=False)`` in fp32 on the same cases, the shape table, and the
tolerance rule.

The rule: the code under test may differ from the fp64 restatement by at most 4 times the largest difference torch's
fp32 optimizer shows to the same restatement over the same cases (``reference_errors``: one figure each for the
parameters, the first and the second moments, after 1 and after 5 steps).  Neither side of that figure involves the
code under test.  ``reference_errors`` asserts that each figure is non-zero, so the allowance is never 0.

The learning rate is 2^-7: the device word is fp32, and a rate that is exact in fp32 keeps the restatement, torch and
the kernel on the same number."""
import functools

import numpy as np
import torch

LR = 2.0 ** -7
BETAS = (0.9, 0.999)
EPS = 1e-8
STEPS = 5
# counts of the tensors of a case: sets of 1, 2, 6 and 8 from {1, 3, 4, 5, 7, 64, 193, 255, 256, 257, 1023, 4097}.
# 4 elements are a unit, 1024 units a chunk, k_refit_one takes up to ONE_CHUNKS_MAX chunks: the totals go across unit
# tails, tensor boundaries inside a chunk, chunk (workgroup) boundaries and the form threshold.
TABLE = [
    (1,), (3,), (4,), (5,), (7,), (64,), (193,), (255,), (256,), (257,), (1023,), (4097,),
    (1, 3), (4, 5), (7, 64), (255, 257), (1023, 4097), (4097, 4097),
    (1, 3, 4, 5, 7, 64), (193, 255, 256, 257, 1023, 4097), (4097, 4097, 4097, 4097, 1, 3), (4097, 1023, 7, 4097, 5, 4097),
    (1, 3, 4, 5, 7, 64, 193, 255), (256, 257, 1023, 4097, 1, 3, 4, 5), (4097, 4097, 4097, 4097, 4097, 7, 193, 1023),
    (4097, 1, 4097, 3, 4097, 5, 4097, 4097),
]
# (max_norm, weight_decay): clip active, clip on but never active (c == 1), no clip; decay 0 and 0.01
HYPERS = [(0.5, 0.0), (0.5, 0.01), (None, 0.0), (None, 0.01), (1e9, 0.01)]
UNIT, CHUNK_UNITS, ONE_CHUNKS_MAX = 4, 1024, 2


def units(counts):
    return sum(-(-n // UNIT) for n in counts)


def chunks(counts):
    return -(-units(counts) // CHUNK_UNITS)


def form_name(counts):
    return "k_refit_one" if chunks(counts) <= ONE_CHUNKS_MAX else "k_refit_norm+k_refit_apply"


def case(i, counts):
    """``(params, grads[step])`` of case i as fp32 numpy arrays: parameters ~ N(0, 1), gradients ~ 0.1 N(0, 1) with a
    scale of their own per step, so the clip at 0.5 is active for the larger cases and idle for the smallest."""
    rng = np.random.default_rng(7000 + i)
    ps = [rng.standard_normal(n).astype(np.float32) for n in counts]
    gs = [[(0.1 * (1 + s) * rng.standard_normal(n)).astype(np.float32) for n in counts] for s in range(STEPS)]
    return ps, gs


def step64(P, G, M, V, t, lr, betas, eps, wd, max_norm):
    """One update in fp64, in place on the lists of fp64 arrays ``P``, ``M``, ``V``; returns the norm."""
    b1, b2 = betas
    norm = float(np.sqrt(sum(float((g.astype(np.float64) ** 2).sum()) for g in G)))
    c = min(1.0, max_norm / (norm + 1e-6)) if max_norm is not None and max_norm > 0 else 1.0
    t1 = t + 1
    for p, g, m, v in zip(P, G, M, V):
        gc = c * g.astype(np.float64)
        p *= 1.0 - lr * wd
        m[:] = b1 * m + (1.0 - b1) * gc
        v[:] = b2 * v + (1.0 - b2) * gc * gc
        p -= (lr / (1.0 - b1 ** t1)) * m / (np.sqrt(v) / np.sqrt(1.0 - b2 ** t1) + eps)
    return norm


def run64(ps, gs, max_norm, wd, steps=STEPS, lr=LR):
    """``{steps done: (P, M, V)}`` after 1 and after ``steps`` updates of the fp64 restatement."""
    P = [p.astype(np.float64) for p in ps]
    M, V = [np.zeros_like(p) for p in P], [np.zeros_like(p) for p in P]
    out = {}
    for s in range(steps):
        step64(P, gs[s], M, V, s, lr, BETAS, EPS, wd, max_norm)
        if s + 1 in (1, steps):
            out[s + 1] = tuple([a.copy() for a in group] for group in (P, M, V))
    return out


def run_torch(ps, gs, max_norm, wd, steps=STEPS, lr=LR):
    """The same with torch's fp32 ``clip_grad_norm_`` and ``AdamW(foreach=False)`` on the CPU."""
    P = [torch.from_numpy(p.copy()).requires_grad_() for p in ps]
    opt = torch.optim.AdamW(P, lr=lr, betas=BETAS, eps=EPS, weight_decay=wd, foreach=False)
    out = {}
    for s in range(steps):
        for p, g in zip(P, gs[s]):
            p.grad = torch.from_numpy(g.copy())
        if max_norm is not None:
            torch.nn.utils.clip_grad_norm_(P, max_norm, foreach=False)
        opt.step()
        if s + 1 in (1, steps):
            out[s + 1] = ([p.detach().numpy().copy() for p in P],
                          [opt.state[p]["exp_avg"].numpy().copy() for p in P],
                          [opt.state[p]["exp_avg_sq"].numpy().copy() for p in P])
    return out


def errors(got, want):
    """``[p, m, v]``: the largest absolute difference of each group of ``got`` (fp32 arrays) to ``want`` (fp64)."""
    return [max(float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(ga, gb)) for ga, gb in zip(got, want)]


def cases(table=TABLE):
    """``(i, counts, max_norm, wd)``: every entry of the table, the hyper-parameters rotated against it."""
    return [(i, counts) + HYPERS[i % len(HYPERS)] for i, counts in enumerate(table)]


@functools.lru_cache(maxsize=None)
def want64(i, counts, max_norm, wd):
    ps, gs = case(i, counts)
    return run64(ps, gs, max_norm, wd)


@functools.lru_cache(maxsize=None)
def reference_errors(table=tuple(TABLE)):
    """``{steps done: [p, m, v]}``: torch's fp32 optimizer against the restatement, the largest over the cases of
    ``table``.  Every figure must be non-zero: 4 times it is what the code under test is allowed."""
    worst = {1: [0.0, 0.0, 0.0], STEPS: [0.0, 0.0, 0.0]}
    for i, counts, max_norm, wd in cases(list(table)):
        ps, gs = case(i, counts)
        ref = run_torch(ps, gs, max_norm, wd)
        for k, want in want64(i, counts, max_norm, wd).items():
            worst[k] = [max(a, b) for a, b in zip(worst[k], errors(ref[k], want))]
    assert all(e > 0.0 for figures in worst.values() for e in figures), worst
    return worst
