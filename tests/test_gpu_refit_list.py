"""``ftn_refit_update_list`` behind ``runtime.refit_update_list`` on the MI355X: a list of one record against
``ftn_refit_update`` bit for bit, eleven tensors - a record boundary after the eighth, sizes across unit tails and chunk
boundaries - against the fp64 restatement of tests/refit_oracle.py within what tests/test_gpu_refit_update.py allows
``ftn_refit_update``, the bytes around every operand, a NaN-poisoned workspace between guards, a skipped call, and the
update captured in a HIP graph and replayed twice.

Every accuracy case prints ``REFIT_ERR`` with its figures."""
import numpy as np
import pytest
import torch

import refit_oracle as oracle
import ws_poison
from test_gpu_refit_update import Run, _same

pytestmark = pytest.mark.gpu

# 1, 5, 4095, 4097 and 3 * 4096 + 1 elements are in: a unit tail, a chunk boundary inside a tensor, and the record
# boundary after the eighth tensor
ELEVEN = (4097, 1, 3, 4, 5, 7, 4095, 193, 3 * 4096 + 1, 255, 1023)
LIST_TABLE = (ELEVEN,) * len(oracle.HYPERS)                       # every (max_norm, weight_decay) of the oracle once


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a ROCm device"
    return torch.device("cuda:0")


class ListRun(Run):
    def call(self, s, grads=None, **kw):
        self.rt.refit_update_list(self.p, self.grads(s) if grads is None else grads, self.m, self.v, self.lr,
                                  self.state, oracle.BETAS, oracle.EPS, self.wd, self.max_norm, log=self.log, **kw)


@pytest.mark.parametrize("i,counts", [(3, (5,)), (15, (255, 257)), (19, (193, 255, 256, 257, 1023, 4097)),
                                      (24, (4097, 4097, 4097, 4097, 4097, 7, 193, 1023))])
def test_a_list_of_one_record_is_refit_update(i, counts, ftn, dev):
    a, b = ListRun(ftn, dev, i, counts, 0.05, 0.01), Run(ftn, dev, i, counts, 0.05, 0.01)
    for s in range(3):
        a.call(s)
        b.call(s)
    assert _same(a.bits(), b.bits()) and torch.equal(a.log, b.log) and torch.equal(a.state, b.state)


@pytest.mark.parametrize("i,counts,max_norm,wd", oracle.cases(list(LIST_TABLE)))
def test_eleven_tensors_against_the_fp64_restatement(i, counts, max_norm, wd, ftn, dev):
    ref = oracle.reference_errors(LIST_TABLE)
    want = oracle.want64(i, counts, max_norm, wd)
    run = ListRun(ftn, dev, i, counts, max_norm, wd)
    run.snapshot()
    for s in range(oracle.STEPS):
        run.call(s)
        if s + 1 in want:
            err = oracle.errors(run.host(), want[s + 1])
            print(f"REFIT_ERR list case {i} after {s + 1}: |p| |m| |v| {err}, torch's own {ref[s + 1]}")
            assert all(e <= 4.0 * r for e, r in zip(err, ref[s + 1]))
    run.around_is_untouched()
    assert run.state.tolist() == [oracle.STEPS, oracle.STEPS]
    log = run.log.cpu()
    norms = [np.sqrt(sum(float((g.astype(np.float64) ** 2).sum()) for g in run.gs[s])) for s in range(oracle.STEPS)]
    np.testing.assert_allclose(log[:oracle.STEPS, 1].numpy(), norms, rtol=1e-6)
    assert log[:oracle.STEPS, 2].tolist() == [oracle.LR] * oracle.STEPS and not log[:oracle.STEPS, 3].any()
    assert not log[oracle.STEPS:].any()


def test_runs_repeat_and_a_poisoned_workspace_changes_nothing(ftn, dev):
    rt = ftn.runtime
    runs = []
    for poisoned in (False, False, True):
        run = ListRun(ftn, dev, 1, ELEVEN, 0.05, 0.01)
        run.snapshot()
        log = []
        with pytest.MonkeyPatch.context() as mp:
            if poisoned:
                mp.setattr(rt, "_workspace", ws_poison.poisoned_workspace(0xFF, log))
            for s in range(3):
                run.call(s)
            if poisoned:
                assert ws_poison.check_guards(log) == 3
                # the first eight tensors are 1025 + 1 + 1 + 1 + 2 + 2 + 1024 + 49 = 2105 units: 3 chunks; the last
                # three 3073 + 64 + 256 = 3393 units: 4 chunks
                assert log[0][1] == 8 * (3 + 4) + 16
        run.around_is_untouched()
        assert all(bool(torch.isfinite(t).all()) for t in run.p + run.m + run.v)
        runs.append(run.bits() + [run.log.clone().view(torch.int32)])
    assert _same(runs[0], runs[1]) and _same(runs[1], runs[2])
    assert float(run.log[0, 1]) > 0.05                          # the clip was active


def test_a_skipped_call_keeps_every_bit_of_all_eleven(ftn, dev):
    run = ListRun(ftn, dev, 2, ELEVEN, 0.05, 0.01, log_steps=16)
    word = lambda v: torch.tensor([v], dtype=torch.int32, device=dev)
    loss = lambda v: torch.tensor([v], device=dev)
    run.call(0, loss=loss(1.5), skip=[word(0)])
    before = run.bits()
    run.snapshot()
    nan_g = run.grads(1)
    nan_g[9][100] = float("nan")                                 # in the second record
    triggers = [(dict(skip=[word(1)]), 1), (dict(skip=[word(0), word(7)], range_mask=2), 4), (dict(grads=nan_g), 8),
                (dict(loss=loss(float("inf"))), 8)]
    for kw, _ in triggers:
        kw.setdefault("loss", loss(2.5))
        run.call(1, **kw)
    assert _same(run.bits(), before)
    run.around_is_untouched()
    assert run.state.tolist() == [1, 1 + len(triggers)]
    assert run.log.cpu()[:1 + len(triggers), 3].tolist() == [0.0] + [float(f) for _, f in triggers]
    run.call(1)
    twin = ListRun(ftn, dev, 2, ELEVEN, 0.05, 0.01)
    twin.call(0)
    twin.call(1)
    assert _same(run.bits(), twin.bits()) and run.state.tolist() == [2, 2 + len(triggers)]


def test_the_update_is_captured_and_replayed_twice(ftn, dev):
    """Three eager calls against one eager call, a capture and two replays on the same gradients."""
    eager, graphed = ListRun(ftn, dev, 4, ELEVEN, 0.05, 0.01), ListRun(ftn, dev, 4, ELEVEN, 0.05, 0.01)
    grads = graphed.grads(0)
    ws = torch.empty(8 * (3 + 4) + 16, dtype=torch.uint8, device=dev)
    for _ in range(3):
        eager.call(0, grads=grads)
    graphed.call(0, grads=grads, workspace=ws)                   # the first call, not captured
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        graphed.call(0, grads=grads, workspace=ws)
    torch.cuda.synchronize()
    assert graphed.state.tolist() == [1, 1]                      # capturing ran nothing
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert _same(graphed.bits(), eager.bits()) and torch.equal(graphed.log, eager.log)
    assert graphed.state.tolist() == eager.state.tolist() == [3, 3]


def test_device_adamw_list_takes_the_hip_backend(ftn, dev):
    fit = ftn.fit
    ps, gs = oracle.case(0, ELEVEN)
    P = [torch.nn.Parameter(torch.from_numpy(p.copy()).to(dev)) for p in ps]
    opt = fit.DeviceAdamWList(P, lr=oracle.LR, betas=oracle.BETAS, eps=oracle.EPS, weight_decay=0.01, max_norm=0.05)
    run = ListRun(ftn, dev, 0, ELEVEN, 0.05, 0.01)
    for s in range(2):
        opt.step_on([torch.from_numpy(g).to(dev) for g in gs[s]])
        run.call(s)
        assert fit._last_optim_backend == "hip"
    assert all(torch.equal(a.detach(), b) for a, b in zip(P + opt.exp_avg + opt.exp_avg_sq, run.p + run.m + run.v))
    assert opt.state_dict()["t"] == 2 and opt.history().shape == (2, 4)
