"""Scoring on the MI355X (``ftn_score_columns`` / ``ftn_score_fold`` behind ``score.negative_binomial_nll`` and
``score.ForecastScorer``): per-element accuracy of the log-likelihood against fp64 with the reference's own fp32
formula as the yardstick, sums that add nothing to it, bit-reproducibility (run to run, row alone or in a batch, one
update or two, every id layout), the edges (non-finite values in and out of the mask, everything masked, negative y,
zero rate, ids out of range) and a TimesNet forward feeding the scorer without a synchronisation.

The accuracy criterion: e = max |ll - ll64| / mag over the valid elements, mag the sum of the magnitudes of the five
addends, both in fp64 on the CPU from the same inputs; e_ref the same figure of the reference's fp32 formula run with
torch on the CPU; asserted e <= 2 e_ref + 2 u (u = 2^-24).  Every case prints ``SCORE_ERR`` with both figures."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
U = 2.0 ** -24

SHAPES = [(1, 1, 1), (3, 7, 5), (2, 5, 8), (4, 24, 37), (2, 96, 64), (5, 7, 1)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a ROCm device"
    return torch.device("cuda:0")


def _draw(shape, seed, regime="mixed"):
    """The issue's distribution: rate = exp(U(-4, 8)), y ~ Poisson(min(rate, 1e4)), a 20 % mask; dispersion
    exp(U(log 1e-3, 2)) ("mixed"), exp(U(log 1e-6, log 1e-3)) ("small") or as mixed with y up to 1e6 ("large")."""
    g = torch.Generator().manual_seed(seed)
    rate = torch.exp(torch.rand(shape, generator=g) * 12.0 - 4.0)
    lo, hi = (np.log(1e-6), np.log(1e-3)) if regime == "small" else (np.log(1e-3), 2.0)
    disp = torch.exp(torch.rand(shape, generator=g) * (hi - lo) + lo)
    y = torch.poisson(rate.clamp(max=1e4), generator=g)
    if regime == "large":
        y = torch.floor(torch.exp(torch.rand(shape, generator=g) * np.log(1e6)))
        rate = rate * 100.0
    mask = torch.rand(shape, generator=g) >= 0.2
    return y, rate, disp, mask


def _ll64(y, rate, disp, eps=1e-8):
    """(ll, mag) in fp64 from the fp32 inputs, clamped as the fp32 formula clamps them."""
    yc = torch.clamp(y, min=0.0).double()
    al = torch.clamp(disp, min=eps).double()
    mu = torch.clamp(rate, min=eps).double()
    l1p, r = torch.log1p(al * mu), 1.0 / al
    terms = [torch.lgamma(yc + r), -torch.lgamma(r), -torch.lgamma(yc + 1.0), -r * l1p,
             yc * (torch.log(al) + torch.log(mu) - l1p)]
    return sum(terms), sum(t.abs() for t in terms)


def _valid(y, rate, disp, mask):
    v = torch.isfinite(torch.clamp(y, min=0.0)) & torch.isfinite(rate.clamp(min=1e-8)) & torch.isfinite(disp.clamp(min=1e-8))
    return v if mask is None else v & (mask != 0)


def _err(ll, ll64, mag, valid):
    if not bool(valid.any()):
        return 0.0
    return float(((ll.double() - ll64).abs() / mag)[valid].max())


def _views(ftn, part):
    sums, counts = ftn.score._part_views(part)
    return sums.cpu(), counts.cpu()


def _check_case(ftn, dev, y, rate, disp, mask, tag, dy=None, dmask=None):
    """Accuracy through ll_out, the column sums against the fp64 ascending-h sums of ll_out / of the fp32 terms, the
    counts, and the scalar of negative_binomial_nll.  ``dy`` / ``dmask``: the device operands when they are special
    views; otherwise plain copies."""
    rt, sc = ftn.runtime, ftn.score
    B, H, N = y.shape
    dy = y.to(dev) if dy is None else dy
    dr, dd = rate.to(dev), disp.to(dev)
    dmask = (None if mask is None else mask.to(dev)) if dmask is None else dmask
    form = rt.score_form(dy, dr, dd, dmask)
    part, ll = rt.score_columns(dy, dr, dd, dmask, want_ll=True)
    ll = ll.cpu()
    valid = _valid(y, rate, disp, mask)
    ll64, mag = _ll64(y, rate, disp)
    e = _err(ll, ll64, mag, valid)
    ll_ref = sc._nb_ll_torch(y, rate, disp, 1e-8)[0]
    e_ref = _err(ll_ref, ll64, mag, valid)
    print(f"SCORE_ERR {tag} {form[0]} nseg={form[1]} shape={(B, H, N)} e={e / U:.3f}u e_ref={e_ref / U:.3f}u")
    assert e <= 2 * e_ref + 2 * U, (tag, form, e / U, e_ref / U)
    assert bool((ll[~valid] == 0).all())
    sums, counts = _views(ftn, part)
    neg = torch.where(valid, -ll, torch.zeros_like(ll)).double()
    terms, cnt = sc._smape_terms_torch(y, rate, valid)
    want = torch.zeros(B, N, 2, dtype=torch.float64)
    for h in range(H):
        want[..., 0] += neg[:, h]
        want[..., 1] += terms[:, h].double()
    got = sums.view(B, N, 2)
    assert bool(((got - want).abs() <= 1e-13 * want.abs()).all()), (tag, float((got - want).abs().max()))
    assert torch.equal(counts.view(B, N, 2)[..., 0].long(), valid.sum(1))
    assert torch.equal(counts.view(B, N, 2)[..., 1].long(), cnt.sum(1))
    nll = sc.negative_binomial_nll(dy, dr, dd, dmask)
    assert sc._last_backend == "hip" and nll.dim() == 0
    den = max(int(valid.sum()), 1)
    want_nll = float(-(ll64[valid]).sum()) / den
    bound = (2 * e_ref + 2 * U) * float(mag[valid].sum()) / den
    assert abs(float(nll) - want_nll) <= bound, (tag, float(nll), want_nll, bound)
    return form, part


@pytest.mark.parametrize("maskkind", ["none", "bool", "fp32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_accuracy_and_sums(shape, maskkind, ftn, dev):
    y, rate, disp, m = _draw(shape, seed=sum(shape) + len(maskkind))
    mask = {"none": None, "bool": m, "fp32": m.float() * 2.5}[maskkind]
    form, _ = _check_case(ftn, dev, y, rate, disp, mask, f"mixed/{maskkind}")
    assert form[0] == ("k_score_cols<4>" if shape[2] % 4 == 0 else "k_score_cols<1>")
    assert form[1] == -(-shape[1] // max(4, -(-shape[1] // 8)))


@pytest.mark.parametrize("regime", ["small", "large"])
@pytest.mark.parametrize("shape", [(4, 24, 37), (2, 96, 64)], ids=["scalar", "vector"])
def test_accuracy_small_dispersion_and_large_counts(shape, regime, ftn, dev):
    y, rate, disp, m = _draw(shape, seed=7 + sum(shape), regime=regime)
    _check_case(ftn, dev, y, rate, disp, m, regime)


def test_views_of_y_take_the_scalar_form(ftn, dev):
    """y offset by one element, and y with a batch stride that is no multiple of 4: vector -> scalar form, same
    records as the plain copy."""
    rt = ftn.runtime
    B, H, N = 2, 5, 8
    y, rate, disp, m = _draw((B, H, N), seed=3)
    _, plain = _check_case(ftn, dev, y, rate, disp, m, "plain")
    buf = torch.zeros(B * H * N + 1, device=dev)
    buf[1:] = y.to(dev).reshape(-1)
    off = buf[1:].view(B, H, N)
    form, part = _check_case(ftn, dev, y, rate, disp, m, "offset", dy=off)
    assert form[0] == "k_score_cols<1>" and torch.equal(part, plain)
    wide = torch.zeros(B, H * N + 2, device=dev)
    wide[:, :H * N] = y.to(dev).reshape(B, -1)
    strided = wide[:, :H * N].view(B, H, N)
    assert strided.stride(0) == H * N + 2
    form, part = _check_case(ftn, dev, y, rate, disp, m, "strided", dy=strided)
    assert form[0] == "k_score_cols<1>" and torch.equal(part, plain)
    wide4 = torch.zeros(B, H * N + 4, device=dev)
    wide4[:, :H * N] = y.to(dev).reshape(B, -1)
    form, part = _check_case(ftn, dev, y, rate, disp, m, "strided4", dy=wide4[:, :H * N].view(B, H, N))
    assert form[0] == "k_score_cols<4>" and torch.equal(part, plain)


def _cpu_fold(sums, counts, B, N, ids, n_slots):
    """acc[slot] += part[b, n] in ascending (b, n) order, on the host."""
    acc_s, acc_c = np.zeros((n_slots, 2)), np.zeros((n_slots, 2), np.int64)
    s, c = sums.numpy().reshape(B, N, 2), counts.numpy().reshape(B, N, 2)
    for b in range(B):
        for n in range(N):
            slot = n if ids is None else int(ids[n] if ids.ndim == 1 else ids[b, n])
            acc_s[slot] += s[b, n]
            acc_c[slot] += c[b, n]
    return acc_s, acc_c


@pytest.mark.parametrize("shape", [(3, 7, 5), (4, 24, 36), (5, 7, 1)], ids=["scalar", "vector", "pipeline"])
def test_reproducibility_and_id_layouts(shape, ftn, dev):
    rt, sc = ftn.runtime, ftn.score
    B, H, N = shape
    y, rate, disp, m = (t.to(dev) for t in _draw(shape, seed=11 + N))
    part, ll = rt.score_columns(y, rate, disp, m, want_ll=True)
    again, ll2 = rt.score_columns(y, rate, disp, m, want_ll=True)
    assert torch.equal(part, again) and torch.equal(ll, ll2)                    # run to run
    for b in range(B):                                                          # a row alone = the row in the batch
        alone, _ = rt.score_columns(y[b:b + 1], rate[b:b + 1], disp[b:b + 1], m[b:b + 1].contiguous())
        assert torch.equal(alone, part.view(B, N * 24)[b]), b
    sums, counts = _views(ftn, part)
    S = N + 3
    g = torch.Generator().manual_seed(5)
    layouts = {"none": None, "shared": torch.arange(N) + 2, "permuted": torch.randperm(S, generator=g)[:N],
               "per_sample": torch.randint(0, S, (B, N), generator=g)}
    for name, ids in layouts.items():
        one, two = sc.ForecastScorer(S, dev), sc.ForecastScorer(S, dev)
        dids = None if ids is None else ids.to(dev)
        per_sample = ids is not None and ids.dim() == 2
        cat = lambda t: torch.cat([t, t.flip(0)])
        one.update(y, rate, disp, m, dids)
        one.update(y.flip(0), rate.flip(0), disp.flip(0), m.flip(0), dids.flip(0) if per_sample else dids)
        two.update(cat(y), cat(rate), cat(disp), cat(m), cat(dids) if per_sample else dids)
        assert one._last_backend == "hip"
        r1, r2 = one.result(), two.result()
        for k in ("nll_sum", "smape_sum", "nll_count", "smape_count"):
            assert np.array_equal(r1[k], r2[k]), (name, k)                      # X then Y = cat([X, Y])
        s2 = torch.cat([sums.view(B, N, 2), sums.view(B, N, 2).flip(0)]).reshape(-1, 2)
        c2 = torch.cat([counts.view(B, N, 2), counts.view(B, N, 2).flip(0)]).reshape(-1, 2)
        ids2 = ids if ids is None or ids.dim() == 1 else torch.cat([ids, ids.flip(0)])
        acc_s, acc_c = _cpu_fold(s2, c2, 2 * B, N, None if ids2 is None else ids2.numpy(), S)
        assert np.array_equal(r1["nll_sum"], acc_s[:, 0]) and np.array_equal(r1["smape_sum"], acc_s[:, 1]), name
        assert np.array_equal(r1["nll_count"], acc_c[:, 0]) and np.array_equal(r1["smape_count"], acc_c[:, 1]), name


def test_edges(ftn, dev):
    sc, rt = ftn.score, ftn.runtime
    shape = (3, 7, 8)
    y, rate, disp, m = _draw(shape, seed=21)
    m[0, 1, 2] = m[1, 3, 4] = m[2, 5, 6] = False
    base = sc.negative_binomial_nll(y.to(dev), rate.to(dev), disp.to(dev), m.to(dev))
    part0, _ = rt.score_columns(y.to(dev), rate.to(dev), disp.to(dev), m.to(dev))
    y2, r2, d2 = y.clone(), rate.clone(), disp.clone()
    y2[0, 1, 2], r2[1, 3, 4], d2[2, 5, 6] = float("nan"), float("inf"), float("-inf")
    poisoned = sc.negative_binomial_nll(y2.to(dev), r2.to(dev), d2.to(dev), m.to(dev))
    part1, _ = rt.score_columns(y2.to(dev), r2.to(dev), d2.to(dev), m.to(dev))
    assert sc._last_backend == "hip"
    assert bool(torch.isfinite(poisoned)) and torch.equal(poisoned, base) and torch.equal(part0, part1)
    # unmasked non-finite elements: dropped by the finite test, and the counts show it
    part2, ll2 = rt.score_columns(y2.to(dev), r2.to(dev), torch.where(torch.isfinite(d2), d2, torch.full_like(d2, float("nan"))).to(dev),
                                  want_ll=True)
    _, counts = _views(ftn, part2)
    assert int(counts[:, 0].sum()) == y.numel() - 3 and bool(torch.isfinite(ll2).all())
    sums, _ = _views(ftn, part2)
    assert bool(torch.isfinite(sums).all())
    # everything masked
    s = sc.ForecastScorer(8, dev)
    s.update(y.to(dev), rate.to(dev), disp.to(dev), torch.zeros(shape, dtype=torch.bool, device=dev))
    r = s.result()
    assert r["nll"] == 0.0 and r["smape"] == 0.0 and r["nll_count"].sum() == 0
    assert float(sc.negative_binomial_nll(y.to(dev), rate.to(dev), disp.to(dev), torch.zeros(shape, device=dev))) == 0.0
    # negative y: clamped for the likelihood only; rate == 0: mu = eps
    yn, r0 = y.clone(), rate.clone()
    yn[:, 0] = -3.0
    r0[:, 1] = 0.0
    partn, lln = rt.score_columns(yn.to(dev), r0.to(dev), disp.to(dev), want_ll=True)
    ll64, mag = _ll64(yn, r0, disp)
    assert _err(lln.cpu(), ll64, mag, torch.ones(shape, dtype=torch.bool)) <= 2 * U + 2 * _err(
        sc._nb_ll_torch(yn, r0, disp, 1e-8)[0], ll64, mag, torch.ones(shape, dtype=torch.bool))
    sums, counts = _views(ftn, partn)
    terms, cnt = sc._smape_terms_torch(yn, r0, torch.ones(shape, dtype=torch.bool))
    assert torch.equal(counts.view(3, 8, 2)[..., 1].long(), cnt.sum(1))
    assert float(terms[:, 0].min()) > 0 and bool(torch.isfinite(sums).all())
    want = terms.double().sum(1)
    assert bool(((sums.view(3, 8, 2)[..., 1] - want).abs() <= 1e-13 * want.abs()).all())
    # an id out of range raises from result(); nothing was written for it
    bad = sc.ForecastScorer(8, dev)
    bad.update(y.to(dev), rate.to(dev), disp.to(dev), None, torch.tensor([0, 1, 2, 3, 4, 5, 6, 8], device=dev))
    with pytest.raises(ValueError, match="outside"):
        bad.result()
    bad2 = sc.ForecastScorer(8, dev)
    ids = (torch.arange(24) % 8).view(3, 8)
    ids[1, 2] = -1
    bad2.update(y.to(dev), rate.to(dev), disp.to(dev), None, ids.to(dev))
    with pytest.raises(ValueError, match="outside"):
        bad2.result()
    with pytest.raises(ValueError, match="mask must be contiguous"):
        rt.score_columns(y.to(dev), rate.to(dev), disp.to(dev), torch.ones(3, 7, dtype=torch.bool, device=dev))


def test_model_forward_feeds_the_scorer_without_a_synchronisation(ftn, dev):
    """A tiny TimesNet (d_model 16, 2 blocks, HIP heads) -> update; eval_metrics over three batches against the CPU
    torch backend on copies of the same rate / dispersion; an event recorded after the last update is still pending
    or done by itself - update() never waited for it."""
    sc = ftn.score
    L, H, N, B = 24, 6, 24, 4
    cfg = dict(input_len=L, pred_len=H, d_model=16, d_ff=32, n_layers=2, k_periods=3, kernel_set=[(3, 3), (5, 5)],
               dropout=0.0, activation="gelu", mode="direct", use_checkpoint=False)
    g = torch.Generator().manual_seed(1)
    torch.manual_seed(0)
    model = ftn.models.TimesNet(**cfg).eval()
    with torch.no_grad():
        model(torch.rand(2, L, N, generator=g) + 1.0)
        for p in model.parameters():
            if float(p.abs().sum()) == 0.0:
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
    model = model.to(dev)
    t = torch.arange(L, dtype=torch.float32).view(1, L, 1)
    batches, outs = [], []
    for i in range(3):
        x = torch.rand(B, L, N, generator=g) + 1.5 + torch.sin(2 * torch.pi * t / 6.0)
        yb = torch.poisson(torch.full((B, H, N), 2.0), generator=g)
        batches.append((x, yb, (torch.rand(B, H, N, generator=g) >= 0.2).float()))
    scorer = sc.ForecastScorer(N, dev)
    with torch.inference_mode():
        for x, yb, mk in batches:
            rate, disp = model(x.to(dev))
            assert model._last_head_backend == "hip"
            outs.append((rate, disp))
        staged = [(yb.to(dev), mk.to(dev) > 0) for _, yb, mk in batches]
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")                 # any synchronising torch call raises from here on
        try:
            for (yb, mk), (rate, disp) in zip(staged, outs):
                scorer.update(yb, rate, disp, mk)
            ev = torch.cuda.Event()
            ev.record()
            done_at_once = ev.query()                           # a query, not a wait: legal while the work is pending
        finally:
            torch.cuda.set_sync_debug_mode("default")
    assert scorer._last_backend == "hip" and isinstance(done_at_once, bool)
    ev.synchronize()
    assert ev.query()
    res = scorer.result()
    via = sc.eval_metrics(model, batches, "direct", H, use_loss_mask=True, n_series=N)
    assert via["nll"] == res["nll"] and via["smape"] == res["smape"] and np.array_equal(via["nll_sum"], res["nll_sum"])
    cpu = sc.ForecastScorer(N, "cpu")
    num = den = 0.0
    for (x, yb, mk), (rate, disp) in zip(batches, outs):
        rate, disp = rate.cpu(), disp.cpu()
        cpu.update(yb, rate, disp, mk > 0)
        valid = _valid(yb, rate, disp, mk)
        ll64, mag = _ll64(yb, rate, disp)
        e_ref = _err(sc._nb_ll_torch(yb, rate, disp, 1e-8)[0], ll64, mag, valid)
        num += (2 * e_ref + 2 * U) * float(mag[valid].sum())
        den += float(valid.sum())
    want = cpu.result()
    assert abs(res["nll"] - want["nll"]) <= 2 * num / den              # both sides are within the bound of fp64
    assert abs(res["smape"] - want["smape"]) <= 8 * U
    assert np.array_equal(res["nll_count"], want["nll_count"]) and np.array_equal(res["smape_count"], want["smape_count"])
