"""S3-S5 of the period selector on the MI355X (``finalize_body`` of csrc/ftn_finalize.h, launched as ``k_finalize`` and
``k_finalize_pw``) against the host on crafted median spectra: no DFT, one launch and one descriptor copy per case.

The device averages the batch in fp64 and the reference in fp32, so the inputs make the reference's answer unambiguous:
  exact cases  entries are integer multiples of 2^-10, B is a power of two and B * max <= 2^14: both means are exact.
               Ties are planted at 16 (the 1e-8 log1p penalty is below half an ulp: the lowest bin wins) and at 2^-10 over
               a zero background (the penalty decides: ascending bins again).
  gap cases    any B; the batch means form a ladder whose neighbours differ by > 1.5e-3 relative; the gap of the
               reference's own top k + 1 scores, >= 1e-3 between all neighbours, is asserted as a precondition.
Expected values: ``orc.period_select_from_median`` for the picks, ``lib.desc_from_periods`` (flags unset) or
``grouping.PeriodGrouper`` (TIMES_PERIOD_MAX_UNIQ / TIMES_PERIOD_BINNING) for the groups, the softmax-scatter of
``orc.group_weights`` in fp64 for the weights.  Every integer of the descriptor is compared bit for bit; amplitudes are
bit-equal to the gathered columns (rounded for act_dtype 1 / 2); columns beyond the live ones are 0 in both arrays.

The weight bound is not a constant: the error of the fp32 ``orc.group_weights`` against fp64 is measured on the same
inputs (in u = 2^-24 for fp32, 2^-9 for bf16, 2^-11 for fp16 weights), and the kernel must stay within 4 x the maximum
of that over the table (its expf and its summation order may each cost an ulp more than torch's).
"""
import os

import numpy as np
import pytest
import torch

import oracle.timesblock_oracle as orc

pytestmark = pytest.mark.gpu
KMAX = 16
Q = 2.0 ** -10
UNIT = {0: 2.0 ** -24, 1: 2.0 ** -9, 2: 2.0 ** -11}
HALF = {0: torch.float32, 1: torch.bfloat16, 2: torch.float16}
LS = (2, 3, 4, 5, 30, 31, 32, 33, 96, 510, 511, 512, 513, 514, 1024)
CLAMPS = ("L,1", "16,5", "1,1", "L,L", "3,7")
BIG = 3e38 * Q
INT_FIELDS = ("sel_freq", "sel_period", "sel_group", "g_period", "g_pad", "g_cycles", "g_px_off", "g_tw", "g_th",
              "g_ntx", "g_nty", "g_tile_off")
SCALARS = ("n_sel", "n_groups", "total_px", "tiles_per_row")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a ROCm device"
    return torch.device("cuda:0")


def _clamp(spec, L):
    a, b = spec.split(",")
    return (L if a == "L" else int(a)), (L if b == "L" else int(b))


def _planted(F):
    """Bin 1, bin F - 1, the run of adjacent high bins below it (they share ceil(L / i): duplicate periods) and a few
    bins between, in the order their scores shall descend."""
    want = [1, F - 1, F - 2, F - 3, F - 4, 2, 3, F // 2, F // 3, 5, 7, F // 2 + 1, 11, 13, F // 4, 17, 19, 23]
    out = []
    for f in want:
        if 1 <= f < F and f not in out:
            out.append(f)
    return out


# ---------------------------------------------------------------------------------------------------------- inputs
def exact_med(L, B, ties, tiny, seed):
    """[B, F] multiples of 2^-10 with exact batch means.  ``tiny``: the first ``ties`` planted bins average 2^-10 over a
    zero background; otherwise they average 16 over distinct background means in (0, 2.1)."""
    F = L // 2 + 1
    g = torch.Generator().manual_seed(seed)
    mean = torch.zeros(F, dtype=torch.float64)
    bins = _planted(F)[:ties]
    if tiny:
        mean[bins] = Q
    else:
        mean[torch.randperm(F, generator=g)] = (torch.arange(F, dtype=torch.float64) + 1.0) * 4.0 * Q
        mean[bins] = 16.0
    med = mean.repeat(B, 1)
    if B > 1:            # rows differ: +d on even rows, -d on odd ones, d a multiple of 2^-10 that keeps 0 <= entry <= 2^14 / B
        room = torch.minimum(mean, torch.full_like(mean, 2.0 ** 14 / B) - mean).clamp_min(0.0)
        d = torch.floor(torch.rand(F, generator=g, dtype=torch.float64) * (room / Q + 1.0)).clamp_max_(room / Q) * Q
        sign = torch.where(torch.arange(B) % 2 == 0, 1.0, -1.0).to(torch.float64).view(B, 1)
        med = med + sign * d
    assert float(med.min()) >= 0.0 and float(med.max()) * B <= 2.0 ** 14 and B & (B - 1) == 0
    assert torch.equal(med.sum(0) / B, mean) and torch.equal(med.float().double(), med)
    return med.float()


def ladder_med(L, B, n_top, scale, seed, ratio=None):
    """[B, F] whose batch means are ``scale`` x a shuffled ladder 0.2 .. 1.0 (neighbours > 1.5e-3 apart, relative), the
    planted bins on its top rungs in planted order (``ratio``: a geometric ladder ``ratio ** j`` for those instead);
    rows scatter +-30 % around the mean with the scatter centred over the batch."""
    F = L // 2 + 1
    g = torch.Generator().manual_seed(seed)
    bins = _planted(F)[:n_top]
    rest = [f for f in range(F) if f not in bins]
    rest = [rest[i] for i in torch.randperm(len(rest), generator=g).tolist()]
    rung = torch.zeros(F, dtype=torch.float64)
    order = bins + rest                                         # descending mean
    rung[order] = 0.2 + 0.8 * (F - 1 - torch.arange(F, dtype=torch.float64)) / max(F - 1, 1)
    if ratio is not None:
        rung[bins] = 2.0 * ratio ** torch.arange(len(bins), dtype=torch.float64)
    noise = torch.rand(B, F, generator=g, dtype=torch.float64) - 0.5
    noise = noise - noise.mean(0, keepdim=True)
    return (scale * rung * (1.0 + 0.6 * noise)).float()


# ------------------------------------------------------------------------------------------------------- reference
def _weights(amps, mapping, G, dtype):
    """``orc.group_weights`` with the softmax in ``dtype`` (the oracle's own is fixed to fp32)."""
    valid = [j for j, m in enumerate(mapping) if m >= 0]
    sm = torch.softmax(amps[:, valid].to(dtype), dim=1)
    w = torch.zeros(amps.shape[0], G, dtype=dtype)
    for col, j in enumerate(valid):
        w[:, mapping[j]] += sm[:, col]
    return w


def _flag_gaps(periods, amps, L, lo, hi, log_base):
    """The reference-side margins of the flagged grouping: the smallest relative distance between two group scores
    (batch mean of the members' logsumexp) and between the two largest member means of a group, in fp64."""
    cand = [j for j, p in enumerate(periods) if lo <= p <= hi and (L + (-L) % p) // p >= 2]
    if not cand:
        return float("inf")
    key = lambda p: p if not log_base else int(np.floor(np.log(np.float32(p)) / np.float32(np.log(log_base)) + 1e-6))
    keys = [key(periods[j]) for j in cand]
    a = amps.double()
    scores, margin = [], float("inf")
    for k in sorted(set(keys)):
        members = [cand[i] for i, kk in enumerate(keys) if kk == k]
        scores.append(float(torch.logsumexp(a[:, members], dim=1).mean()))
        if len(members) > 1:
            m = sorted(a[:, members].mean(0).tolist(), reverse=True)
            margin = min(margin, (m[0] - m[1]) / abs(m[0]))
    s = sorted(scores, reverse=True)
    for x, y in zip(s, s[1:]):
        margin = min(margin, (x - y) / abs(x))
    return margin


def expected(ftn, c):
    """The host's answer for case ``c``: descriptor fields, amplitudes, weights in fp64 and in the reference's own
    precision, and the margins the case relies on."""
    L, act = c["L"], c["act"]
    med_all = c["med_all"]                                     # the whole (global) batch; this rank holds med_all[:B]
    B = c["B"]
    pmax, thr = c["pmax"], c["thr"]
    pmax_c = max(1, pmax)
    lo = min(pmax_c, max(1, thr))
    r = orc.period_select_from_median(med_all, L, c["K"], pmax, thr)
    n = len(r.periods)
    e = {"gap": r.topk_gap, "n_sel": n}
    amps = med_all[:B][:, r.freq_idx].to(HALF[act]) if n else torch.zeros(B, 0, dtype=HALF[act])
    flagged = c["mu"] > 0 or c["lb"] > 1.0
    if not flagged:
        hd = ftn.lib.desc_from_periods(r.periods, L, lo, pmax_c)
        mapping = list(hd.sel_group[:n])
    else:
        grouping = ftn.grouping
        old = {v: os.environ.get(v) for v in ("TIMES_PERIOD_MAX_UNIQ", "TIMES_PERIOD_BINNING")}
        try:
            os.environ["TIMES_PERIOD_MAX_UNIQ"] = str(c["mu"]) if c["mu"] > 0 else ""
            os.environ["TIMES_PERIOD_BINNING"] = repr(c["lb"]) if c["lb"] > 1.0 else ""
            for v in old:
                if not os.environ[v]:
                    del os.environ[v]
            gp = grouping.PeriodGrouper(torch.tensor(r.periods, dtype=torch.long), amps.float(), L, min_period=lo,
                                        max_period=pmax_c)
            assert gp.max_unique == (c["mu"] or None) and gp.log_base == (c["lb"] if c["lb"] > 1.0 else None)
            grp = gp.group()
        finally:
            for v, val in old.items():
                os.environ.pop(v, None)
                if val is not None:
                    os.environ[v] = val
        hd = ftn.lib.desc_from_periods(grp.periods.tolist(), L, 1, 2 ** 30)
        assert hd.n_groups == grp.periods.numel()
        mapping = grp.mapping.tolist()
        e["flag_margin"] = _flag_gaps(r.periods, amps, L, lo, pmax_c, c["lb"] if c["lb"] > 1.0 else 0.0)
    G = int(hd.n_groups)
    for fld in INT_FIELDS:
        e[fld] = list(getattr(hd, fld))
    e["sel_freq"] = r.freq_idx + [0] * (KMAX - n)
    e["sel_period"] = r.periods + [0] * (KMAX - n)
    e["sel_group"] = mapping + [-1] * (KMAX - n)
    e.update(n_groups=G, total_px=int(hd.total_px), tiles_per_row=int(hd.tiles_per_row))
    e["amps"] = amps.float()
    e["w64"] = _weights(amps.double(), mapping, G, torch.float64)
    e["wref"] = orc.group_weights(amps, mapping, G).double() if G else torch.zeros(B, 0, dtype=torch.float64)
    e["ref_err"] = float((e["wref"] - e["w64"]).abs().max()) / UNIT[act] if G else 0.0
    return e


# ----------------------------------------------------------------------------------------------------------- table
def _case(kind, L, B, K, clamp, med_all, act=0, mu=0, lb=0.0, nparts=1, name=""):
    pmax, thr = _clamp(clamp, L)
    return dict(kind=kind, L=L, B=B, K=K, pmax=pmax, thr=thr, med_all=med_all, act=act, mu=mu, lb=lb, nparts=nparts,
                name=name or f"{kind} L={L} B={B} K={K} clamp={clamp} act={act} mu={mu} lb={lb} parts={nparts}")


def build_table():
    T = []
    KS, BX = (1, 5, 16, 3), (1, 2, 64, 256, 1024)
    for i, L in enumerate(LS):
        F = L // 2 + 1
        for j, tiny in enumerate((False, True)):
            K = KS[(i + j) % 4]
            B = BX[(i + 2 * j) % 5]
            ties = min(F - 1, (3, 7, 20)[(i + j) % 3])
            # act_dtype 1 / 2 round the scores: only where every pick is one of the ties at 16, which no rounding moves
            act = (0, 0, 1, 2)[(i + j) % 4] if not tiny and K <= ties else 0
            T.append(_case("exact", L, B, K, CLAMPS[(i + 3 * j) % 5], exact_med(L, B, ties, tiny, 100 * i + j), act=act))
    # K = 0, K beyond F - 1, every clamp at one length on both sides of the switch
    T.append(_case("exact", 96, 2, 0, "L,1", exact_med(96, 2, 3, False, 1)))
    T.append(_case("exact", 5, 2, 5, "L,1", exact_med(5, 2, 2, False, 2)))
    T.append(_case("exact", 30, 64, 16, "L,1", exact_med(30, 64, 15, True, 3)))
    for cl in CLAMPS:
        T.append(_case("exact", 510, 2, 16, cl, exact_med(510, 2, 9, False, 4)))
        T.append(_case("exact", 514, 256, 16, cl, exact_med(514, 256, 9, True, 5)))
    # gap cases: any B, partial sums of a larger global batch, amplitude scales
    BG, PARTS, SC = (1, 2, 64, 255, 256, 257, 1024), (1, 2, 3, 8), (1e-3, 1.0, 1e4, BIG)
    for i, L in enumerate(LS):
        B = BG[i % 7]
        nparts = PARTS[i % 4] if B <= 257 else 2
        K = (1, 5, 16)[i % 3]
        scale = SC[i % 4] if B * nparts <= 512 else SC[i % 3]
        T.append(_case("gap", L, B, K, CLAMPS[(2 * i) % 5], ladder_med(L, B * nparts, min(K + 1, L // 2), scale, 300 + i),
                       nparts=nparts))
    for i, B in enumerate(BG):                                   # every B on both top-k forms at K = 16
        for L in (510, 1024):
            T.append(_case("gap", L, B, 16, "L,1", ladder_med(L, B, 17, SC[(i + L) % 3], 400 + i + L)))
    for i, scale in enumerate(SC):                               # every scale with act_dtype 0
        T.append(_case("gap", 96, 3, 5, "L,1", ladder_med(96, 3, 6, scale, 500 + i)))
    # half-precision roundings: batch means a power of two apart, so no rounding of a score moves a pick; the last
    # four put the finite scales other than 1 under both roundings (top mean 4e4: inside fp16's range with its scatter)
    HALVES = ((96, 1, 8.0), (96, 2, 8.0), (510, 1, 8.0), (514, 2, 8.0), (33, 1, 8.0), (1024, 2, 8.0),
              (96, 1, 4e-3), (96, 2, 4e-3), (96, 1, 4e4), (96, 2, 4e4))
    for i, (L, act, top) in enumerate(HALVES):
        F = L // 2 + 1
        bins = _planted(F)[:6]
        mean = torch.full((F,), top * 2.0 ** -9)
        mean[bins] = (top * 0.5 ** torch.arange(6.0))[:len(bins)]
        g = torch.Generator().manual_seed(600 + i)
        B = (2, 64, 4)[i % 3]
        sign = torch.where(torch.arange(B) % 2 == 0, 1.0, -1.0).view(B, 1)
        med = mean + sign * mean * 0.37 * torch.rand(F, generator=g)
        T.append(_case("half", L, B, min(5, len(bins) - 1), CLAMPS[i % 2], med.float(), act=act,
                       name=f"half L={L} B={B} act={act} top={top}"))
    # flagged grouping: more groups than the fixtures' 2-3, every max_unique x log_base, K = 8 and 16
    i = 0
    for K in (8, 16):
        for mu in (0, 1, 2, 4):
            for lb in (0.0, 2.0, 1.5, 1.1):
                L, B = ((96, 2), (510, 64), (1024, 257), (513, 3))[i % 4]
                T.append(_case("flags", L, B, K, "L,1", ladder_med(L, B, K, (1.0, 3.0, 1e4)[i % 3], 706 + i, ratio=0.75),
                               mu=mu, lb=lb))
                i += 1
    return T


@pytest.fixture(scope="module")
def table(ftn):
    T = build_table()
    for c in T:
        c["exp"] = expected(ftn, c)
    return T


def _psum(c, nparts=None):
    """[F] or [nparts, F] fp64 partial sums of the global batch, in row blocks (the last one takes the remainder)."""
    nparts = c["nparts"] if nparts is None else nparts
    m = c["med_all"].double()
    if nparts == 1:
        return m.sum(0)
    edges = [round(i * m.shape[0] / nparts) for i in range(nparts + 1)]
    return torch.stack([m[a:b].sum(0) for a, b in zip(edges, edges[1:])])


def _run(ftn, dev, c, psum=None, stage_a=None):
    rt = ftn.runtime
    med = c["med_all"][:c["B"]].contiguous().to(dev)
    ps = (_psum(c) if psum is None else psum).to(dev)
    sel = rt.finalize(ps, c["med_all"].shape[0], med, c["L"], c["K"], c["pmax"], c["thr"], c["act"], c["mu"], c["lb"],
                      stage_a=stage_a)
    d = sel.host()
    return sel, d, sel.amps.cpu(), sel.weights.cpu()


def _check(c, sel, d, amps, wts, bound):
    e, name = c["exp"], c["name"]
    for fld in SCALARS:
        assert int(getattr(d, fld)) == e[fld], (name, fld, int(getattr(d, fld)), e[fld])
    for fld in INT_FIELDS:
        assert list(getattr(d, fld)) == e[fld], (name, fld, list(getattr(d, fld)), e[fld])
    assert d.total_px <= sel.px_bound and d.n_groups <= sel.max_groups, (name, d.total_px, sel.px_bound)
    n, G = e["n_sel"], e["n_groups"]
    assert torch.equal(amps[:, :n], e["amps"]), name
    assert bool((amps[:, n:] == 0).all()) and bool((wts[:, G:] == 0).all()), name        # dead columns hold 0
    assert bool(torch.isfinite(wts).all()), name
    if G:
        w = wts[:, :G].double()
        rows = (w.sum(1) - 1.0).abs().max()
        # the n roundings of the softmax terms and of their sum, then one per scatter-add
        assert float(rows) <= (n + G) * UNIT[c["act"]], (name, float(rows))
        err = float((w - e["w64"]).abs().max()) / UNIT[c["act"]]
        assert err <= bound[c["act"]], (name, err, bound)
        return err
    return 0.0


@pytest.fixture(scope="module")
def bound(table):
    """4 x the largest error of the reference's own precision against fp64 over the table, per weight dtype."""
    worst = {a: max(c["exp"]["ref_err"] for c in table if c["act"] == a) for a in (0, 1, 2)}
    assert all(v > 0 for v in worst.values())
    print("\nFINALIZE_WEIGHTS reference-side max error [u]:", {a: round(v, 3) for a, v in worst.items()})
    return {a: 4.0 * v for a, v in worst.items()}


MEASURED = {}


@pytest.mark.parametrize("kind", ["exact", "gap", "half", "flags"])
def test_descriptor_amplitudes_and_weights(kind, table, bound, ftn, dev):
    cases = [c for c in table if c["kind"] == kind]
    assert cases
    for c in cases:
        e = c["exp"]
        # The preconditions are asserted wherever a pick or a group depends on them.  The gap is infinite, and nothing
        # to assert, only where the reference ranks nothing out: the clamps leave no candidate, or K >= F - 1 takes
        # every bin.  A "flags" row with both flags unset takes the plain grouping, which compares no scores.
        if kind == "gap" and np.isfinite(e["gap"]):
            scores = _top_scores(c)
            assert all((a - b) / abs(a) >= 1e-3 for a, b in zip(scores, scores[1:])), (c["name"], scores)
        if kind == "flags" and (c["mu"] > 0 or c["lb"] > 1.0):
            assert e["flag_margin"] >= 1e-3, (c["name"], e["flag_margin"])
        err = _check(c, *_run(ftn, dev, c), bound)
        MEASURED[c["act"]] = max(MEASURED.get(c["act"], 0.0), err)
    print(f"\nFINALIZE_WEIGHTS kind={kind} kernel max error [u] per act_dtype so far: "
          f"{ {a: round(v, 3) for a, v in MEASURED.items()} } bound { {a: round(v, 3) for a, v in bound.items()} }")


def _top_scores(c):
    """The reference's own k + 1 largest scores (fp32, penalty applied), descending."""
    m = c["med_all"].mean(0)
    s = m - (1e-8 * torch.log1p(torch.arange(m.numel(), dtype=torch.float32)))
    k = min(max(c["K"], 0), m.numel() - 1)
    return torch.sort(s[1:], descending=True).values[:k + 1].tolist()


def test_expected_picks_of_the_exact_cases(table):
    """The reference side alone: ties resolve to ascending bins (what the exact cases are built to show)."""
    seen = 0
    for c in table:
        if c["kind"] != "exact" or c["K"] <= 0 or c["exp"]["n_sel"] != min(c["K"], c["L"] // 2):
            continue
        F = c["L"] // 2 + 1
        mean = c["med_all"].double().mean(0)
        top = float(mean[1:].max())
        tied = [f for f in range(1, F) if float(mean[f]) == top]
        k = min(c["K"], len(tied))
        assert c["exp"]["sel_freq"][:k] == sorted(tied)[:k], c["name"]
        seen += 1
    assert seen >= 10


def test_three_routes_agree_byte_for_byte(table, bound, ftn, dev):
    """``ftn_period_finalize``, the fused ``ftn_period_finalize_stage_a`` of a small bottleneck block (C = 16), and -
    exact cases - the same sums split over 3 parts: the same descriptor, amplitudes and weights, byte for byte."""
    blk = ftn.models.TimesBlock(d_model=16, d_ff=32, kernel_set=[(3, 3)], dropout=0.0, activation="gelu",
                                bottleneck_ratio=2.0).to(dev).eval()
    wblob, plan = blk._packed(dev)
    assert ftn.runtime.fuse_stage_a(plan)
    ran = 0
    for c in table:
        if c["B"] * c["L"] > 64 * 1024:
            continue
        base = _run(ftn, dev, c)
        ref = (bytes(base[1]), base[2], base[3])
        x = torch.zeros(c["B"], c["L"], 16, device=dev)
        fused = _run(ftn, dev, c, stage_a=ftn.runtime.StageA(x, plan, wblob))
        assert fused[0].stage_a is not None, c["name"]
        got = (bytes(fused[1]), fused[2], fused[3])
        assert got[0] == ref[0] and torch.equal(got[1], ref[1]) and torch.equal(got[2], ref[2]), c["name"]
        if c["kind"] == "exact" and c["nparts"] == 1 and c["B"] >= 2:
            tot = _psum(c, 1)
            third = torch.floor(tot / 3.0 / Q) * Q                # multiples of 2^-10: the three parts sum exactly
            parts = torch.stack([third, third, tot - 2.0 * third])
            assert torch.equal(parts.sum(0), tot)
            split = _run(ftn, dev, c, psum=parts)
            got = (bytes(split[1]), split[2], split[3])
            assert got[0] == ref[0] and torch.equal(got[1], ref[1]) and torch.equal(got[2], ref[2]), c["name"]
        ran += 1
    assert ran >= 40
