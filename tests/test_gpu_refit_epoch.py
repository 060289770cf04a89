"""``ftn_refit_epoch_end`` / ``ftn_refit_epoch_restore`` on the device (``csrc/refit_epoch.hip``): the gated copy
kernel against ``torch.equal`` with guard words around every destination, and the decide kernel against the
plain-Python ``refit_epoch_oracle.EpochOracle`` to the bit, on the sequences of the host test."""
import pytest
import torch

from refit_epoch_oracle import SEQUENCES, EpochOracle, bits, validation_means

pytestmark = pytest.mark.gpu

K = 4096                                                            # elements of a copy chunk
GUARD = 4                                                           # floats before and after every destination


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a ROCm device"
    return torch.device("cuda:0")


class Words:
    """The device words one ``ftn_refit_epoch_end`` reads and writes, for ``n_slots`` slots."""

    def __init__(self, ftn, dev, n_slots, max_epochs, lr=1e-2):
        self.ftn, self.dev = ftn, dev
        self.acc = torch.zeros(n_slots * 24, dtype=torch.uint8, device=dev)
        self.err = torch.zeros(1, dtype=torch.int32, device=dev)
        self.den_extra = torch.zeros(1, dtype=torch.float64, device=dev)
        self.count_seen = torch.zeros(1, dtype=torch.int64, device=dev)
        self.state = torch.zeros(64, dtype=torch.uint8, device=dev)
        self.state.view(torch.float64)[:3] = float("inf")
        self.state.view(torch.float64)[3] = lr
        self.lr = torch.full((1,), lr, dtype=torch.float32, device=dev)
        self.log = torch.zeros(max_epochs, 5, dtype=torch.float64, device=dev)

    def load(self, nll_sum, nll_cnt, smape_sum, smape_cnt, den_extra=0.0):
        n = len(nll_sum)
        host = torch.zeros(n * 24, dtype=torch.uint8)
        sums, counts = self.ftn.score._part_views(host)
        sums[:, 0] = torch.tensor(nll_sum, dtype=torch.float64)
        sums[:, 1] = torch.tensor(smape_sum, dtype=torch.float64)
        counts[:, 0] = torch.tensor(nll_cnt, dtype=torch.int32)
        counts[:, 1] = torch.tensor(smape_cnt, dtype=torch.int32)
        self.acc.copy_(host)
        self.den_extra.fill_(den_extra)
        self.count_seen.fill_(7)

    def end(self, patience=None, plateau=None, src=(), dst=()):
        self.ftn.runtime.refit_epoch_end(self.acc, self.err, self.den_extra, self.count_seen, self.state, self.lr,
                                         self.log, patience, plateau, src, dst)

    def ints(self):
        return self.state.view(torch.int32)[8:15].tolist()

    def doubles(self):
        return self.state.view(torch.float64)[:4].tolist()


def _carve(dev, counts, offsets, seed):
    """Sources of random bits and destinations inside one patterned buffer, destination i starting ``offsets[i]``
    floats past a 16-byte boundary with GUARD floats on either side."""
    g = torch.Generator().manual_seed(seed)
    srcs, spans, at = [], [], 0
    for n, off in zip(counts, offsets):
        at = (at + 3) // 4 * 4 + 4 + off                           # a boundary, a unit of guard, the offset
        spans.append((at, n))
        at += n + GUARD
    buf = torch.arange(at + GUARD, dtype=torch.float32, device=dev) * -1.0 - 0.5
    for (a, n), off in zip(spans, offsets):
        assert (buf[a:].data_ptr() % 16) // 4 == off % 4
        base = torch.randint(-2 ** 31, 2 ** 31 - 1, (n + 8,), generator=g, dtype=torch.int64).to(torch.int32)
        srcs.append(base.view(torch.float32).to(dev)[off % 4:off % 4 + n] if off % 4 else
                    base.view(torch.float32).to(dev)[:n])
    return srcs, [buf[a:a + n] for a, n in spans], buf, spans


LISTS = {
    "one element": ([1], [0]),
    "three elements": ([3], [0]),
    "4k + 1 elements": ([4 * 9 + 1], [0]),
    "eight mixed tensors": ([5, 80, 16, 5, 64, 4, 96, 1], [0] * 8),
    "a view 4 bytes off the grid": ([37, 8], [1, 0]),
    "views 8 and 12 bytes off": ([6, 11], [2, 3]),
    "across a chunk boundary": ([K - 3, K + 9], [0, 0]),
    "one tensor of three chunks, off the grid": ([2 * K + 5], [1]),
}


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("name", list(LISTS))
def test_keep_and_restore_copy_exactly_what_the_gate_allows(name, ftn, dev):
    rt = ftn.runtime
    counts, offsets = LISTS[name]
    if name == "across a chunk boundary":
        assert rt.refit_epoch_form_of(counts) == ("vec", 0, 3)
        assert rt.refit_epoch_form_of([K - 3]) == ("vec", 0, 1)      # the second tensor starts inside chunk 0
    if name == "one tensor of three chunks, off the grid":
        assert rt.refit_epoch_form_of(counts, [4]) == ("mixed", 1, 3)
    srcs, dsts, buf, spans = _carve(dev, counts, offsets, seed=len(name))
    pattern = buf.clone()
    w = Words(ftn, dev, 2, 4)
    # restore on a fresh record (best_epoch = 0): nothing moves
    rt.refit_epoch_restore(w.state, srcs, dsts)
    assert _same_bits(buf, pattern)
    # an epoch that does not improve (NaN): nothing moves
    w.load([float("nan"), 0.0], [1, 0], [0.0, 0.0], [0, 0])
    w.end(src=srcs, dst=dsts)
    assert w.ints()[:2] == [1, 0] and w.ints()[5] == 0 and _same_bits(buf, pattern)
    # an epoch that improves: every destination gets its source, every other word of the buffer stays
    w.load([1.5, 0.0], [1, 0], [0.0, 0.0], [0, 0])
    w.end(src=srcs, dst=dsts)
    assert w.ints()[:2] == [2, 2] and w.ints()[5] == 1
    want = pattern.clone()
    for (a, n), s in zip(spans, srcs):
        want[a:a + n] = s
    assert _same_bits(buf, want)
    assert all(_same_bits(d, s) for d, s in zip(dsts, srcs))
    # restore with best_epoch > 0, in the other direction, into a second patterned buffer
    _, back, buf2, _ = _carve(dev, counts, offsets, seed=1)
    pattern2 = buf2.clone()
    rt.refit_epoch_restore(w.state, dsts, back)
    want2 = pattern2.clone()
    for (a, n), s in zip(spans, srcs):
        want2[a:a + n] = s
    assert _same_bits(buf2, want2)


@pytest.mark.parametrize("n_slots", [1, 5, 130])
@pytest.mark.parametrize("name", list(SEQUENCES))
def test_decide_kernel_is_the_oracle_to_the_bit(name, n_slots, ftn, dev):
    values, lr, patience, plateau = SEQUENCES[name]
    w = Words(ftn, dev, n_slots, len(values), lr)
    oracle = EpochOracle(lr, patience, plateau)
    lr32 = float(torch.tensor(lr, dtype=torch.float32))
    for e, v in enumerate(values):
        nll_sum, nll_cnt = [0.0] * n_slots, [0] * n_slots
        nll_sum[-1], nll_cnt[-1] = v, 1
        sm_sum, sm_cnt = [0.0] * n_slots, [0] * n_slots
        sm_sum[0], sm_cnt[0] = 0.25 * (e + 1), 2
        w.load(nll_sum, nll_cnt, sm_sum, sm_cnt)
        w.end(patience, plateau)
        oracle.end(v, 0.125 * (e + 1), lr_word=lr32)
        assert w.ints() == oracle.words(), (name, e)
        assert bits(w.doubles()) == bits(oracle.doubles()), (name, e)
        assert float(w.lr) == float(torch.tensor(oracle.lr, dtype=torch.float32)), (name, e)
        assert not bool(w.acc.any()) and float(w.den_extra) == 0.0 and int(w.count_seen) == 0
    assert [bits(r) for r in w.log.tolist()] == [bits(r) for r in oracle.rows]


@pytest.mark.parametrize("n_slots", [1, 5, 130, 1024, 1025, 2500])
def test_decide_kernel_adds_in_slot_order(n_slots, ftn, dev):
    """Random contents, 1024 records a pass: the sums of ``ForecastScorer.result()``, the error word and den_extra."""
    g = torch.Generator().manual_seed(n_slots)
    nll = (torch.randn(n_slots, generator=g, dtype=torch.float64) * 1e3).tolist()
    sm = torch.rand(n_slots, generator=g, dtype=torch.float64).tolist()
    c0 = torch.randint(0, 50, (n_slots,), generator=g).tolist()
    c1 = torch.randint(0, 50, (n_slots,), generator=g).tolist()
    w = Words(ftn, dev, n_slots, 3)
    w.load(nll, c0, sm, c1, den_extra=20.0)
    w.err.fill_(1)
    w.end()
    a, b = validation_means(nll, c0, sm, c1, 20.0)
    assert bits(w.log[0].tolist()) == bits([a, b, float(w.lr), 32.0, 1.0])
    assert not bool(w.acc.any()) and float(w.den_extra) == 0.0
    w.end()                                                          # nothing accumulated: both means are 0
    assert bits(w.log[1].tolist()) == bits([0.0, 0.0, float(w.lr), 32.0, 1.0 if a > 0.0 else 0.0])
    w.end()
    w.end()                                                          # a call beyond the log writes no row
    assert w.ints()[6] == 4 and w.ints()[0] == 4


def test_epoch_end_matches_its_torch_backend_on_real_batches(ftn, dev):
    """``fit.EpochEnd`` on the device against the CPU torch backend fed the same batches (the device's own scoring
    kernels feed both: the CPU side gets the device accumulators' bytes)."""
    fit = ftn.fit
    g = torch.Generator().manual_seed(9)
    params = [torch.randn(33, generator=g).to(dev), torch.randn(4, 5, generator=g).to(dev)]
    host_params = [p.cpu() for p in params]
    end = fit.EpochEnd(params, 7, 4, 1e-2, patience=1, plateau=dict(factor=0.5, patience=0))
    ref = fit.EpochEnd(host_params, 7, 4, 1e-2, patience=1, plateau=dict(factor=0.5, patience=0), backend="torch")
    opt, ref_opt = fit.DeviceAdamW(params, lr=1e-2), fit.DeviceAdamW(host_params, lr=1e-2, backend="torch")
    plain = ftn.score.ForecastScorer(7, dev)
    for e in range(4):
        for k in range(2):
            y = torch.poisson(torch.full((3, 4, 7), 2.0), generator=g).to(dev)
            rate = (torch.rand(3, 4, 7, generator=g) + 1.5 + 1.5 * e).to(dev)
            disp = (torch.rand(3, 4, 7, generator=g) + 0.1).to(dev)
            mask = (torch.rand(3, 4, 7, generator=g) > (1.0 if k == 1 and e == 1 else 0.3)).to(dev)
            end.accumulators.update(y, rate, disp, mask)
            if e == 0:
                plain.update(y, rate, disp, mask)
        if e == 0:
            assert torch.equal(end.accumulators._acc, plain._acc)
            assert torch.equal(end.accumulators._den_extra, plain._den_extra)
        for name in ("_acc", "_err", "_den_extra", "_count_seen"):
            getattr(ref.accumulators, name).copy_(getattr(end.accumulators, name))
        with torch.no_grad():
            for p, q in zip(params, host_params):
                p.add_(1.0)
                q.add_(1.0)
        end.end_epoch(opt)
        assert fit._last_epoch_backend == "hip"
        ref.end_epoch(ref_opt)
        assert torch.equal(end.state.cpu(), ref.state) and _same_bits(opt._lr.cpu(), ref_opt._lr)
        assert torch.equal(end.log.cpu().view(torch.int64), ref.log.view(torch.int64))
        assert all(torch.equal(a.cpu(), b) for a, b in zip(end.best, ref.best))
    assert bits([plain.result()["nll"], plain.result()["smape"]]) == bits(end.log[0, :2].tolist())
    a, b = end.history(), ref.history()
    assert a["best_epoch"] == b["best_epoch"] >= 1 and a["stopped_epoch"] == b["stopped_epoch"]
    end.restore()
    ref.restore()
    assert all(torch.equal(p.cpu(), q) for p, q in zip(params, host_params))
