"""Batch-sharded multi-GPU TimesBlock forward (one process per GPU, RCCL through
``torch.distributed``).

The reference is single-process; this is new work.  A TimesBlock cannot be sharded
along channels without changing its results (channel median in the selector,
channel-mixing convs), but batch rows are independent once the shared periods are
known.  So every rank owns ``B/world`` rows and the data path needs exactly

1. one tiny exchange per block call: the ``[F]`` fp64 partial batch sums of the
   channel-median spectrum are all-gathered and summed in rank order on every
   rank (deterministic and identical everywhere, unlike a ring all-reduce), which
   makes the selected periods identical on all ranks;
2. optionally one all-gather along ``B`` of the output.

Everything else (top-k, grouping, convs, aggregation) is rank-local.
"""
from __future__ import annotations

import contextlib
import os
from typing import Optional

import torch
import torch.distributed as dist
from torch import nn

from . import range_guard
from .models.shell import hip_width_ok


def _refuse_flagged_grouping(block_index=None) -> None:
    """The reference's TIMES_PERIOD_MAX_UNIQ / TIMES_PERIOD_BINNING grouping variants rank candidate groups by batch
    means of the amplitudes (:374-378, :394-437).  A sharded run exchanges only the [F] spectrum sums, so each rank
    would rank on its own rows and the ranks could keep different groups: refuse instead of diverging silently."""
    from .grouping import _resolve_log_binning_base, _resolve_scheduled_int

    if (_resolve_scheduled_int(os.getenv("TIMES_PERIOD_MAX_UNIQ"), block_index) or
            _resolve_log_binning_base(os.getenv("TIMES_PERIOD_BINNING"), block_index)):
        raise NotImplementedError("TIMES_PERIOD_MAX_UNIQ / TIMES_PERIOD_BINNING are not supported with a batch-sharded "
                                  "selector: unset them or run unsharded")


def _refuse_capture(sharded: bool, x: torch.Tensor, exchange, gather) -> None:
    """A sharded call captured into a HIP graph may use neither a collective (the ``torch.distributed`` all-gather of
    the partial sums, ``gather=True`` / ``"async"``) nor a host-side sequence number (a mode-0 ``IpcExchange``, whose
    captured ``seq`` a replay would reuse: the finalize would read the peers' words of an earlier call).  Raise before
    anything is enqueued instead of capturing a graph that races or hangs."""
    if not sharded or not x.is_cuda or not torch.cuda.is_current_stream_capturing():
        return
    if exchange is None:
        raise RuntimeError("a sharded forward cannot be captured with the torch.distributed exchange (exchange=None): "
                           "use dist.IpcExchange(..., capturable=True)")
    if not exchange.capturable:
        raise RuntimeError("a sharded forward cannot be captured with an IpcExchange built with capturable=False "
                           "(its sequence number is a launch argument): build it with capturable=True")
    if gather:
        raise RuntimeError("a sharded forward cannot be captured with gather=True / 'async' (a collective): capture "
                           "with gather=False and call dist.gather_batch on the outputs after the replay")


@contextlib.contextmanager
def _sharded_selector(sel, group, exchange, sharded: bool, x: torch.Tensor):
    """Point the shared selector at the process group (and the IPC exchange, on the device) for one call."""
    prev = sel.shard_group, sel.shard_exchange
    sel.shard_group = group if sharded else None
    sel.shard_exchange = exchange if (exchange is not None and x.is_cuda) else None
    try:
        yield
    finally:
        sel.shard_group, sel.shard_exchange = prev


class IpcExchange:
    """SURVEY section 8e step 2 without a collective: every rank owns one exchange buffer in its GPU's memory, maps the
    other ranks' buffers once (``hipIpcGetMemHandle`` / ``hipIpcOpenMemHandle``, handles traded through the process
    group), and from then on each block call's partial sums are plain stores into the peers' buffers issued by the
    selector's own kernel, with a sequence word behind them (``include/flowtimes.h``, ``FtnExchange``).  Attach it with
    ``ShardedTimesBlock(block, group, exchange=IpcExchange(group, device))``; ranks must call in lockstep.

    ``capturable=True`` (``FtnExchange.mode`` 1): the sequence number is not a launch argument but a call counter in
    this rank's own buffer, read and advanced by the kernels, so the sharded forward can be captured in a HIP graph
    (``graph.GraphedForward`` with ``gather=False``) and eager calls and replays can be mixed on one exchange.
    ``calls()`` returns that counter."""

    _IPC_HANDLE_BYTES = 64

    def __init__(self, group, device: torch.device, f_cap: int = 1024, capturable: bool = False) -> None:
        import ctypes as C

        from . import lib as _lib

        self.group = group if group is not None else dist.group.WORLD
        self.world, self.rank = dist.get_world_size(self.group), dist.get_rank(self.group)
        if self.world > _lib.FTN_XCHG_MAXWORLD:
            raise ValueError(f"IpcExchange supports up to {_lib.FTN_XCHG_MAXWORLD} ranks")
        self.device = torch.device(device)
        lib = _lib.load()
        nbytes = lib.ftn_exchange_bytes(self.world, int(f_cap))
        if nbytes == 0:
            raise ValueError(f"ftn_exchange_bytes rejected world={self.world} F_cap={f_cap}")
        self._C, self._lib = C, lib
        torch.cuda.set_device(self.device)
        torch.zeros(1, device=self.device)                      # the HIP context of this device exists
        own = C.c_void_p()
        handle = C.create_string_buffer(self._IPC_HANDLE_BYTES)
        _lib.check(lib.ftn_exchange_alloc(self.world, int(f_cap), C.byref(own), handle), "ftn_exchange_alloc")
        handles = [None] * self.world
        dist.all_gather_object(handles, bytes(handle.raw), group=self.group)
        self._own, self._mapped = own, []
        self.x = _lib.FtnExchange()
        self.x.world, self.x.rank, self.x.F_cap, self.x.seq = self.world, self.rank, int(f_cap), 0
        self.capturable = bool(capturable)
        self.x.mode = 1 if self.capturable else 0
        for r, raw in enumerate(handles):
            if r == self.rank:
                self.x.slots[r] = own.value
                continue
            peer = C.c_void_p()
            _lib.check(lib.ftn_exchange_open(C.create_string_buffer(raw, self._IPC_HANDLE_BYTES), C.byref(peer)),
                       f"ftn_exchange_open(rank {r})")
            self._mapped.append(peer)
            self.x.slots[r] = peer.value
        dist.barrier(group=self.group)                          # every rank has zeroed and mapped before the first call

    def next_call(self, F: int):
        """The struct pointer for one exchange (every rank must make the same calls).  Bumps the host sequence number;
        with ``capturable=True`` the device counter is the only one, so nothing changes on the host."""
        if F > self.x.F_cap:
            raise ValueError(f"IpcExchange: F={F} exceeds F_cap={self.x.F_cap}")
        if not self.capturable:
            self.x.seq += 1
        return self._C.byref(self.x)

    def calls(self) -> int:
        """Synchronises; the number of exchanges this rank has completed (``capturable=True`` only): eager calls and
        graph replays alike.  Equal on every rank that called in lockstep."""
        from . import lib as _lib
        from . import runtime

        if not self.capturable:
            raise RuntimeError("IpcExchange.calls() needs capturable=True (mode 0 counts on the host: x.seq)")
        n = _lib.load().ftn_exchange_calls(self._C.byref(self.x), runtime._stream(self.device))
        if n < 0:
            raise RuntimeError(f"ftn_exchange_calls failed: {_lib.load().ftn_last_error().decode(errors='replace')}")
        return int(n)

    def check(self) -> None:
        """Synchronises; raises if a peer's sums did not arrive within the kernel's bounded wait."""
        from . import lib as _lib
        from . import runtime

        rc = _lib.load().ftn_exchange_error(self._C.byref(self.x), runtime._stream(self.device))
        if rc != 0:
            raise RuntimeError("IpcExchange: a peer's partial sums did not arrive (timeout)" if rc == 1
                               else f"ftn_exchange_error rc={rc}")

    def close(self) -> None:
        torch.cuda.synchronize(self.device)
        dist.barrier(group=self.group)                          # nobody still writes into a buffer that is going away
        for peer in self._mapped:
            self._lib.ftn_exchange_close(peer)
        self._mapped = []
        if self._own is not None:
            self._lib.ftn_exchange_free(self._own)
            self._own = None


def gather_batch(y_local: torch.Tensor, group=None, async_op: bool = False):
    """All-gather equal-sized shards along dim 0 -> ``[world*B_local, ...]`` on every rank.

    ``async_op=True`` returns ``(out, work)``: the collective runs on the backend's own stream
    (RCCL over xGMI) and overlaps whatever the caller enqueues next; ``work.wait()`` makes the
    current stream wait for it.  ``out`` must not be read before that."""
    world = dist.get_world_size(group)
    if world == 1 and os.environ.get("FTN_BENCH_FORCE_DIST") != "1":
        return (y_local, None) if async_op else y_local
    y_local = y_local.contiguous()
    out = y_local.new_empty((world * y_local.shape[0],) + tuple(y_local.shape[1:]))
    if y_local.is_cuda and dist.get_backend(group) != "gloo":
        work = dist.all_gather_into_tensor(out, y_local, group=group, async_op=async_op)
    else:  # gloo (CPU tests)
        parts = list(out.chunk(world, dim=0))
        work = dist.all_gather(parts, y_local, group=group, async_op=async_op)
    return (out, work) if async_op else out


class ShardedTimesBlock(nn.Module):
    """Wraps a ``TimesBlock`` (with an ``FFTPeriodSelector``) for batch-sharded use.

    ``forward(x_local)`` returns this rank's rows (``gather=False``) or the
    re-assembled global batch (``gather=True``).  Shards must be equally sized.

    f16x2 range guard: the block repairs a flagged call on its own rank (``check_range()``, its next call), on the
    selection the call made, so no exchange is repeated and the ranks stay in lockstep.  With ``gather=True`` /
    ``"async"`` the all-gather is enqueued before that repair, so the gathered copy can hold the unrepaired rows.
    """

    def __init__(self, block: nn.Module, group=None, exchange: Optional[IpcExchange] = None) -> None:
        super().__init__()
        self.block = block
        self.group = group
        self.exchange = exchange                                 # None: all-gather through torch.distributed (RCCL / gloo)
        sel = block.period_selector
        if sel is None or not hasattr(sel, "shard_group"):
            raise ValueError("ShardedTimesBlock needs a block with a native FFTPeriodSelector")

    def forward(self, x_local: torch.Tensor, gather=True):
        """``gather``: ``False`` -> this rank's rows; ``True`` -> the re-assembled global batch;
        ``"async"`` -> ``(out, work)`` with the all-gather still in flight (see ``gather_batch``),
        which lets a serving loop overlap step i's output exchange with step i+1's compute."""
        sel = self.block.period_selector
        grp = self.group if self.group is not None else dist.group.WORLD
        if dist.get_world_size(grp) > 1:
            _refuse_flagged_grouping(getattr(self.block, "block_index", None))
        sharded = dist.get_world_size(grp) > 1 or os.environ.get("FTN_BENCH_FORCE_DIST") == "1"
        _refuse_capture(sharded, x_local, self.exchange, gather)
        with _sharded_selector(sel, grp, self.exchange, sharded, x_local):
            y = self.block(x_local)
        if gather == "async":
            return gather_batch(y, grp, async_op=True)
        return gather_batch(y, grp) if gather else y


class _ShardedModel(nn.Module):
    """What both whole-model wrappers share: ``graph.GraphedForward`` defers the model's output checks during capture
    and runs them after every replay, through the three attributes forwarded here."""

    @property
    def _defer_checks(self) -> bool:
        return self.model._defer_checks

    @_defer_checks.setter
    def _defer_checks(self, v: bool) -> None:
        self.model._defer_checks = v

    @property
    def _pending_bad(self):
        return self.model._pending_bad

    @_pending_bad.setter
    def _pending_bad(self, v) -> None:
        self.model._pending_bad = v

    def check_outputs(self) -> None:
        self.model.check_outputs()


class ShardedTimesNet(_ShardedModel):
    """Batch-sharded whole model (P2): the model's blocks share one ``FFTPeriodSelector``, so
    pointing its ``shard_group`` at the process group makes every block exchange its ``[F]`` partial sums;
    everything else in ``TimesNet.forward`` is row-wise or per-series and needs no communication.
    ``forward`` returns this rank's ``(rate, dispersion)`` rows, or the all-gathered ones with ``gather=True``.
    ``exchange``: as in ``ShardedTimesBlock``; with ``IpcExchange(..., capturable=True)`` the wrapper can be captured
    by ``graph.GraphedForward(wrapper, x_local, gather=False)``, which runs the model's deferred output checks through
    the three attributes forwarded by ``_ShardedModel``.

    f16x2 range guard: after an eager forward the blocks' flags are all-reduced (MAX) over the group and, if any rank
    tripped, every rank switches its blocks to ``bf16x3`` and repeats the forward, so the ranks stay in lockstep.  In a
    captured forward ``check_outputs()`` raises instead."""

    def __init__(self, model: nn.Module, group=None, exchange: Optional[IpcExchange] = None) -> None:
        super().__init__()
        self.model = model
        self.group = group
        self.exchange = exchange                                 # None: all-gather through torch.distributed (RCCL / gloo)
        if not hasattr(model.period_selector, "shard_group"):
            raise ValueError("ShardedTimesNet needs the mirror TimesNet (native FFTPeriodSelector)")

    def forward(self, x_local: torch.Tensor, gather: bool = False, **kwargs):
        m = self.model
        grp = self.group if self.group is not None else dist.group.WORLD
        if dist.get_world_size(grp) > 1:
            for blk in m.blocks:
                _refuse_flagged_grouping(getattr(blk, "block_index", None))
        sharded = dist.get_world_size(grp) > 1 or os.environ.get("FTN_BENCH_FORCE_DIST") == "1"
        _refuse_capture(sharded, x_local, self.exchange, gather)
        with _sharded_selector(m.period_selector, grp, self.exchange, sharded, x_local):
            # the model's single pass under this wrapper's collective decision (never the model's rank-local one)
            rate, disp = range_guard.repeat_on_trip(
                m.blocks, lambda: m._forward_once(x_local, **kwargs), group=grp if sharded else None,
                message="ShardedTimesNet: a value left the fp16 range of engine f16x2 on some rank; every rank repeats "
                        "the forward on engine bf16x3")
        if not m._defer_checks:
            m.check_outputs()
        if gather:
            return gather_batch(rate, grp), gather_batch(disp, grp)
        return rate, disp


# ---- series (channel) sharding -------------------------------------------------------------------------------------
class IpcRowExchange:
    """Peer-store exchange of fp32 rows (``include/flowtimes.h``, ``FtnRowExchange``): every rank owns one buffer in its
    GPU's memory and maps the others once (handles traded through the process group, as ``IpcExchange``).  Each call
    is one push (``runtime.rowx_push``) and one consume on every rank, in lockstep; the call counter lives in the
    buffer, so eager calls and graph replays can be mixed.

    ``kind="reduce_scatter"``: a rank pushes ``[world * rows_per_rank, width]`` rows, row block q to rank q, and
    ``runtime.rowx_reduce`` sums what arrived in rank order.  ``kind="all_gather"``: a rank pushes
    ``[rows_per_rank, width]`` rows to every rank and ``runtime.rowx_gather`` returns all of them."""

    _IPC_HANDLE_BYTES = 64
    KINDS = {"reduce_scatter": 0, "all_gather": 1}

    def __init__(self, group, device: torch.device, rows_per_rank: int, width: int,
                 kind: str = "reduce_scatter") -> None:
        import ctypes as C

        from . import lib as _lib

        if kind not in self.KINDS:
            raise ValueError(f"IpcRowExchange: kind must be one of {sorted(self.KINDS)}")
        self.group = group if group is not None else dist.group.WORLD
        self.world, self.rank = dist.get_world_size(self.group), dist.get_rank(self.group)
        if self.world > _lib.FTN_XCHG_MAXWORLD:
            raise ValueError(f"IpcRowExchange supports up to {_lib.FTN_XCHG_MAXWORLD} ranks")
        self.device = torch.device(device)
        self.kind = kind
        lib = _lib.load()
        if lib.ftn_rowx_bytes(self.world, int(rows_per_rank), int(width)) == 0:
            raise ValueError(f"ftn_rowx_bytes rejected world={self.world} rows_per_rank={rows_per_rank} width={width}")
        self._C, self._lib = C, lib
        torch.cuda.set_device(self.device)
        torch.zeros(1, device=self.device)                      # the HIP context of this device exists
        own = C.c_void_p()
        handle = C.create_string_buffer(self._IPC_HANDLE_BYTES)
        _lib.check(lib.ftn_rowx_alloc(self.world, int(rows_per_rank), int(width), C.byref(own), handle),
                   "ftn_rowx_alloc")
        handles = [None] * self.world
        dist.all_gather_object(handles, bytes(handle.raw), group=self.group)
        self._own, self._mapped = own, []
        self.x = _lib.FtnRowExchange()
        self.x.world, self.x.rank = self.world, self.rank
        self.x.rows_per_rank, self.x.width, self.x.kind = int(rows_per_rank), int(width), self.KINDS[kind]
        for r, raw in enumerate(handles):
            if r == self.rank:
                self.x.slots[r] = own.value
                continue
            peer = C.c_void_p()
            _lib.check(lib.ftn_rowx_open(C.create_string_buffer(raw, self._IPC_HANDLE_BYTES), C.byref(peer)),
                       f"ftn_rowx_open(rank {r})")
            self._mapped.append(peer)
            self.x.slots[r] = peer.value
        dist.barrier(group=self.group)                          # every rank has zeroed and mapped before the first call
        self.ref = C.byref(self.x)

    @property
    def rows_per_rank(self) -> int:
        return int(self.x.rows_per_rank)

    @property
    def width(self) -> int:
        return int(self.x.width)

    def calls(self) -> int:
        """Synchronises; the exchanges this rank has completed (eager calls and graph replays alike)."""
        from . import runtime

        n = self._lib.ftn_rowx_calls(self.ref, runtime._stream(self.device))
        if n < 0:
            raise RuntimeError(f"ftn_rowx_calls failed: {self._lib.ftn_last_error().decode(errors='replace')}")
        return int(n)

    def check(self) -> None:
        """Synchronises; raises if a peer's rows did not arrive within the kernels' bounded wait."""
        from . import runtime

        rc = self._lib.ftn_rowx_error(self.ref, runtime._stream(self.device))
        if rc != 0:
            raise RuntimeError("IpcRowExchange: a peer's rows did not arrive (timeout)" if rc == 1
                               else f"ftn_rowx_error rc={rc}")

    def close(self) -> None:
        torch.cuda.synchronize(self.device)
        dist.barrier(group=self.group)                          # nobody still writes into a buffer that is going away
        for peer in self._mapped:
            self._lib.ftn_rowx_close(peer)
        self._mapped = []
        if self._own is not None:
            self._lib.ftn_rowx_free(self._own)
            self._own = None


def series_row_exchanges(model: nn.Module, batch: int, group=None, device=None):
    """The two row exchanges of a ``SeriesShardedTimesNet`` forward of ``batch`` rows: the embedding reduce-scatter
    (``[B/W, L*D]`` rows) and the hidden all-gather (``[B/W, H*D]`` rows).  Collective: every rank calls it."""
    grp = group if group is not None else dist.group.WORLD
    world = dist.get_world_size(grp)
    if batch % world:
        raise ValueError(f"batch {batch} is not a multiple of the world size {world}")
    device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    D, L = int(model.requested_d_model), int(model.input_len)
    steps = int(model._out_steps)
    return (IpcRowExchange(grp, device, batch // world, L * D, "reduce_scatter"),
            IpcRowExchange(grp, device, batch // world, steps * D, "all_gather"))


class SeriesShardedTimesNet(_ShardedModel):
    """Series-sharded (channel-sharded) whole model: every rank holds ``[B, T, N_r]``, a contiguous slice of the series
    in rank order (slices may be uneven), and gets ``(rate, dispersion)`` of its own series, ``[B, H, N_r]``.

    Only the value embedding ``Linear(N -> d_model)`` mixes series, so a forward is
    1. a partial embedding over the rank's series (``TimesNet.series_partial_embedding``), ``[B, L, D]``;
    2. a reduce-scatter along B, summed in rank order; value bias, positional / time-feature term and the embedding
       norm are applied once, after the sum (IPC: ``ftn_rowx_reduce``);
    3. the blocks on the rank's ``B/W`` rows, batch-sharded as ``ShardedTimesNet`` (the ``[F]`` exchange);
    4. ``forecast_time_proj`` and an all-gather along B of ``[B/W, H, D]`` (IPC: ``ftn_rowx_gather``);
    5. the heads on the rank's rows of ``mu_head`` / ``sigma_head`` (``TimesNet.series_heads``).

    ``exchange``: the blocks' ``[F]`` exchange (``IpcExchange(..., capturable=True)`` or None for torch.distributed);
    ``row_exchange``: ``(reduce_scatter, all_gather)`` ``IpcRowExchange`` pair (``series_row_exchanges``) or None for
    torch.distributed (gloo or RCCL).  With both IPC exchanges the forward can be captured by
    ``graph.GraphedForward(wrapper, x_local, gather=False)``.

    f16x2 range guard: the blocks flag out-of-range values in a device word; after an eager forward the flags are
    all-reduced (MAX) over the group and, if any rank tripped, every rank switches its blocks to ``bf16x3`` and repeats
    the forward, so the ranks stay in lockstep.  In a captured forward ``check_outputs()`` raises instead."""

    def __init__(self, model: nn.Module, n_series: int, group=None, exchange: Optional[IpcExchange] = None,
                 row_exchange=None) -> None:
        super().__init__()
        self.model = model
        self.n_series = int(n_series)
        self.group = group
        self.exchange = exchange
        self.row_exchange = tuple(row_exchange) if row_exchange is not None else None
        if not hasattr(model.period_selector, "shard_group"):
            raise ValueError("SeriesShardedTimesNet needs the mirror TimesNet (native FFTPeriodSelector)")
        if (model.embedding is None or model.mu_head is None or model.input_channels != self.n_series
                or model.mu_head.out_features != self.n_series
                or model.embedding.value_embedding.in_features != self.n_series):
            raise ValueError(f"the model is not built for n_series={self.n_series}: run one unsharded forward (or load "
                             f"a checkpoint) with all series first, with the same weights on every rank")
        if self.row_exchange is not None and len(self.row_exchange) != 2:
            raise ValueError("row_exchange must be the (reduce_scatter, all_gather) pair of series_row_exchanges")
        self._sizes = None

    def series_sizes(self, n_local: int, grp):
        """Every rank's series count (one collective at the first call; never during a capture)."""
        if self._sizes is None:
            if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("SeriesShardedTimesNet: the series split is learnt at the first eager call, not "
                                   "during a capture")
            sizes = [None] * dist.get_world_size(grp)
            dist.all_gather_object(sizes, int(n_local), group=grp)
            if sum(sizes) != self.n_series or min(sizes) < 1:
                raise ValueError(f"series slices {sizes} do not add up to n_series={self.n_series}")
            self._sizes = [int(s) for s in sizes]
        return self._sizes

    def _refuse(self, x_local: torch.Tensor, sharded: bool, gather) -> None:
        if self.model.training:
            raise RuntimeError("SeriesShardedTimesNet is inference only: call model.eval()")
        if torch.is_grad_enabled() and (x_local.requires_grad or any(p.requires_grad for p in self.model.parameters())):
            raise RuntimeError("SeriesShardedTimesNet is inference only: run it under torch.inference_mode() / "
                               "torch.no_grad()")
        if not (x_local.is_cuda and torch.cuda.is_current_stream_capturing()):
            return
        if self.row_exchange is None:
            raise RuntimeError("a series-sharded forward cannot be captured with the torch.distributed row exchange "
                               "(row_exchange=None): use dist.series_row_exchanges(...)")
        if gather:
            raise RuntimeError("a series-sharded forward cannot be captured with gather=True (a collective): capture "
                               "with gather=False and gather along N after the replay")
        _refuse_capture(sharded, x_local, self.exchange, False)

    def forward(self, x_local: torch.Tensor, x_mark: Optional[torch.Tensor] = None,
                series_static: Optional[torch.Tensor] = None, series_ids: Optional[torch.Tensor] = None,
                gather: bool = False):
        m = self.model
        grp = self.group if self.group is not None else dist.group.WORLD
        world, rank = dist.get_world_size(grp), dist.get_rank(grp)
        if world > 1:
            for blk in m.blocks:
                _refuse_flagged_grouping(getattr(blk, "block_index", None))
        sharded = world > 1 or os.environ.get("FTN_BENCH_FORCE_DIST") == "1"
        self._refuse(x_local, sharded, gather)
        if x_local.dim() != 3:
            raise ValueError("SeriesShardedTimesNet expects x_local shaped [B, T, n_local]")
        B, T, n_local = x_local.shape
        if B % world:
            raise ValueError(f"batch {B} is not a multiple of the world size {world}")
        L = m.input_len
        if T < L:
            raise ValueError(f"Input sequence length {T} is shorter than required input_len {L}")
        if x_mark is not None and tuple(x_mark.shape[:2]) != (B, T):
            raise ValueError("x_mark must share batch/time dimensions with x_local (all B rows)")
        hip = x_local.is_cuda
        if hip:
            D = int(m.d_model)
            if not hip_width_ok(D):
                raise ValueError(f"d_model={D} is outside the HIP kernels' limits (a multiple of 4, <= 128)")
            if x_local.dtype != torch.float32:
                raise ValueError("SeriesShardedTimesNet takes fp32 inputs on the HIP path")
            if m.embedding.embed_norm_mode not in ("none", "layer", "decoupled"):
                raise ValueError(f"embed_norm_mode={m.embedding.embed_norm_mode!r} has no series-sharded HIP path")
        sizes = self.series_sizes(n_local, grp)
        if sizes[rank] != n_local:
            raise ValueError("the series slice changed between calls")
        offset = sum(sizes[:rank])
        window = x_local.narrow(1, T - L, L)
        mark = None if x_mark is None else x_mark.narrow(1, T - L, L)
        sl = m.series_slices(offset, n_local, x_local.device)
        rate, disp, bad = range_guard.repeat_on_trip(
            m.blocks, lambda: self._forward_once(window, mark, series_static, series_ids, sl, offset, grp, world, rank,
                                                 sharded),
            group=grp if sharded else None,
            message="SeriesShardedTimesNet: a value left the fp16 range of engine f16x2 on some rank; every rank "
                    "repeats the forward on engine bf16x3")
        if bad is not None:
            m._pending_bad = bad
            if not m._defer_checks:
                m.check_outputs()
        if gather:
            return self.gather_series(rate, grp), self.gather_series(disp, grp)
        return rate, disp

    def _forward_once(self, window, mark, series_static, series_ids, sl, offset, grp, world, rank, sharded):
        m = self.model
        B, L, _ = window.shape
        Bq = B // world
        rows = m.series_context_rows(window, series_static, series_ids, offset)
        part = m.series_partial_embedding(window, rows, sl["w_emb"])              # [B, L, D]
        D = part.size(-1)
        mark_q = None if mark is None else mark[rank * Bq:(rank + 1) * Bq]
        add, ln = m.series_embedding_epilogue(window, mark_q)
        rx = self.row_exchange if window.is_cuda else None
        if rx is not None:
            from . import runtime

            self._check_row_exchange(rx, Bq, L, D, m._out_steps, world)
            runtime.rowx_push(part, rx[0].ref)
            seq = runtime.rowx_reduce(rx[0].ref, Bq, L, D, window.device, add, ln)
        else:
            summed = self._reduce_scatter(part, grp, world, sharded)
            seq = summed + add
            if ln is not None:
                seq = torch.nn.functional.layer_norm(seq, (D,), ln[0], ln[1], ln[2])
            elif m.embedding.norm is not None:                   # rms (torch path only)
                seq = m.embedding.norm(seq)
        with _sharded_selector(m.period_selector, grp, self.exchange, sharded, window):
            seq = m._stack(seq)
        steps = m._out_steps
        hidden_q = m.series_hidden(seq, steps)                                       # [B/W, steps, D]
        if rx is not None:
            from . import runtime

            runtime.rowx_push(hidden_q, rx[1].ref)
            hidden = runtime.rowx_gather(rx[1].ref, (B, steps, D), window.device)
        elif sharded:
            hidden = self._all_gather_rows(hidden_q, grp, world)
        else:
            hidden = hidden_q
        return m.series_heads(hidden, window, rows, sl, steps)

    @staticmethod
    def _check_row_exchange(rx, Bq: int, L: int, D: int, steps: int, world: int) -> None:
        rs, ag = rx
        if rs.kind != "reduce_scatter" or ag.kind != "all_gather":
            raise ValueError("row_exchange must be (reduce_scatter, all_gather)")
        if rs.world != world or ag.world != world:
            raise ValueError("row_exchange was built for another group")
        if (rs.rows_per_rank, rs.width) != (Bq, L * D) or (ag.rows_per_rank, ag.width) != (Bq, steps * D):
            raise ValueError(f"row_exchange was built for other shapes: want rows_per_rank={Bq}, widths "
                             f"{L * D} / {steps * D}")

    @staticmethod
    def _reduce_scatter(part: torch.Tensor, grp, world: int, sharded: bool) -> torch.Tensor:
        """torch.distributed reduce-scatter along B, summed in rank order: all-to-all of the row blocks, then the
        sum over sources 0..W-1 (gloo moves the rows through host memory)."""
        if not sharded:
            return part
        gloo = dist.get_backend(grp) == "gloo"
        src = part.contiguous()
        if gloo and src.is_cuda:
            src = src.cpu()
        parts = torch.empty_like(src)
        dist.all_to_all_single(parts, src, group=grp)
        parts = parts.to(part.device).view(world, part.size(0) // world, *part.shape[1:])
        acc = parts[0].clone()
        for s in range(1, world):
            acc += parts[s]
        return acc

    @staticmethod
    def _all_gather_rows(y: torch.Tensor, grp, world: int) -> torch.Tensor:
        y = y.contiguous()
        if dist.get_backend(grp) == "gloo":
            host = y.cpu()
            outs = [torch.empty_like(host) for _ in range(world)]
            dist.all_gather(outs, host, group=grp)
            return torch.cat(outs, dim=0).to(y.device)
        out = y.new_empty((world * y.size(0),) + tuple(y.shape[1:]))
        dist.all_gather_into_tensor(out, y, group=grp)
        return out

    def gather_series(self, y: torch.Tensor, grp=None) -> torch.Tensor:
        """All-gather ``[B, H, N_r]`` along N (uneven slices allowed) -> ``[B, H, N]`` on every rank.  Collective;
        not capturable."""
        grp = grp if grp is not None else (self.group if self.group is not None else dist.group.WORLD)
        world = dist.get_world_size(grp)
        sizes = self._sizes
        nmax = max(sizes)
        pad = torch.zeros(y.shape[:-1] + (nmax,), dtype=y.dtype, device=y.device)
        pad[..., :y.size(-1)] = y
        gloo = dist.get_backend(grp) == "gloo"
        if gloo:
            pad = pad.cpu()
        outs = [torch.empty_like(pad) for _ in range(world)]
        dist.all_gather(outs, pad, group=grp)
        return torch.cat([o[..., :n] for o, n in zip(outs, sizes)], dim=-1).to(y.device)
