"""Model shell around the TimesBlock hot path: mirrors of the reference's ``PositionalEmbedding``, ``RMSNorm``,
``DataEmbedding`` and ``TimesNet`` (``models/timesnet.py:1104-1325, 1374-2102`` of the reference) - the same
constructor signatures, attribute names, error messages and ``state_dict`` keys (the checkpoint ABI), and
``forward(x[B,T,N], x_mark, series_static, series_ids) -> (rate, dispersion)``.

SURVEY section 8f ranks 1-2.  The structure is this package's own: the lazily built layers come from one declarative
table (``_LAZY_TABLE``), and the forward is four stages - series context rows, embedding front end, block stack,
heads - each of which calls the HIP entry point for its stage when the tensors live on a ROCm device
(``ftn_embed_forward``, the TimesBlock kernels with the LayerNorm epilogue, ``ftn_timeproj_forward``,
``ftn_head_forward``) and composes stock torch ops otherwise (CPU tensors, autograd, dropout in training).

Each stage has one body, and four callers compose them: the plain forward (``_forward_once``), the device recursive
forecaster (``forecast.py``), the series-sharded forward (``dist.SeriesShardedTimesNet``, through the thin
``series_*`` entry points, which hand the same bodies this rank's slices) and ``head_inputs``, which stops before the
heads for a refit of them (``fit.refit_heads``):

* context rows - ``_rows_of`` (``_context_rows`` / ``series_context_rows`` resolve the ids their own way);
* embedding - ``_context_terms``, then ``_through_weight`` + ``_embed_epilogue`` (HIP) or ``_with_context`` (torch);
* heads - ``_late_bias``, ``_time_projection``, ``_rate_dispersion``.

The context front end of these bodies runs in three launches of ``csrc/context.hip`` on ROCm fp32 tensors without
autograd: ``_rows_of`` -> ``ftn_context_rows`` (the rows carry the coefficients, the constant bias and the late bias,
which ``_context_terms`` and ``_late_bias`` hand back), ``_through_weight`` + ``_embed_epilogue`` ->
``ftn_context_through_weight`` + ``ftn_embed_add`` (``add`` in one pass).  Anything the kernels do not take (other
dtypes, autograd, a LayerNorm without affine parameters, sizes beyond their limits, ``FTN_CTX_HIP=0``) keeps the torch
composition; ``_last_context_backend`` says which ran.

``hip_shell_width_ok`` is the one statement of the d_model these kernels take (up to 512: the narrow entry points up
to 128, the ``ftn_*_wide_*`` ones beyond, chosen in ``runtime``); ``hip_width_ok`` is the narrower limit of the
series-sharded forward's row exchange.
"""
from __future__ import annotations

import math
import os
from typing import Callable, NamedTuple, Optional, Tuple

import torch
import torch.nn.functional as F
from torch import nn
from torch.utils.checkpoint import checkpoint

from .. import range_guard
from .timesnet import (FFTPeriodSelector, LowRankTemporalContext, TimesBlock, _affine_layernorm,
                       _layer_norm_fp32 as _norm, _ln_params, _param_key, _safe_param_dtype)

# the limits of the context kernels (include/flowtimes.h): ctx / F / Ws / Ed, rank, time features
_CTX_MAX, _CTX_RMAX, _ADD_TMAX = 256, 32, 64


def _place(module: nn.Module, ref: torch.Tensor) -> nn.Module:
    """Lazily built modules follow the input's device; parameters stay fp32 for
    half-precision inputs (reference :30-34)."""
    return module.to(device=ref.device, dtype=_safe_param_dtype(ref.dtype))


def hip_width_ok(d_model: int) -> bool:
    """The d_model the narrow shell kernels and the row exchange of the series-sharded forward (``ftn_rowx_*``) take."""
    return d_model % 4 == 0 and d_model <= 128


# FTN_SHELL_WIDE=0 (read once): the shell at d_model > 128 composes torch ops, as before the wide kernels (A/B runs)
_SHELL_WIDE = os.environ.get("FTN_SHELL_WIDE", "1").strip() != "0"


# FTN_CTX_HIP=0 (read once): the context front end (series rows, context terms, the embedding's `add`) composes torch
# ops, as before its kernels (A/B runs)
_CTX_HIP = os.environ.get("FTN_CTX_HIP", "1").strip() != "0"


def hip_shell_width_ok(d_model: int) -> bool:
    """The d_model the shell's HIP kernels (embedding, time projection, heads) take: multiples of 4 up to 512."""
    return d_model % 4 == 0 and d_model <= (512 if _SHELL_WIDE else 128)


# -------------------------------------------------------------------------
# embedding pieces                                       reference :1104-1325
# -------------------------------------------------------------------------
class PositionalEmbedding(nn.Module):
    """Parameter-free sinusoidal encoding ``[sin(t w_0), cos(t w_0), sin(t w_1), ...]``, ``w_i = 10000^(-2i/d)``,
    evaluated in fp32; the table is a pure function of (L, device) and is kept between calls."""

    def __init__(self, d_model: int) -> None:
        super().__init__()
        self.d_model = int(d_model)
        self._table: Optional[Tuple[Tuple[int, str], torch.Tensor]] = None

    def table(self, L: int, device: torch.device) -> torch.Tensor:
        key = (L, str(device))
        if self._table is None or self._table[0] != key or torch.is_grad_enabled():
            d = self.d_model
            rate = torch.exp(torch.arange(0, d, 2, device=device, dtype=torch.float32) * (-math.log(10000.0) / d))
            phase = torch.arange(L, device=device, dtype=torch.float32).unsqueeze(1) * rate          # [L, ceil(d/2)]
            pe = torch.stack((torch.sin(phase), torch.cos(phase)), dim=-1).reshape(L, -1)[:, :d].contiguous()
            self._table = (key, pe)
        return self._table[1]

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.ndim != 3:
            raise ValueError("PositionalEmbedding expects input shaped [B, L, C]")
        return self.table(x.size(1), x.device).to(x.dtype).unsqueeze(0).expand(x.size(0), -1, -1)


class RMSNorm(nn.Module):
    def __init__(self, d_model: int, eps: float = 1e-5) -> None:
        super().__init__()
        if d_model <= 0:
            raise ValueError("RMSNorm expects a positive embedding dimension")
        self.eps = float(eps)
        self.weight = nn.Parameter(torch.ones(int(d_model)))
        self.bias = nn.Parameter(torch.zeros(int(d_model)))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.size(-1) != self.weight.numel():
            raise ValueError("RMSNorm dimension mismatch")
        cd = _safe_param_dtype(x.dtype)
        v = x.to(cd)
        inv_rms = torch.rsqrt(v.square().mean(dim=-1, keepdim=True) + self.eps)
        return torch.addcmul(self.bias.to(cd), v * inv_rms, self.weight.to(cd)).to(x.dtype)


def _affine_rmsnorm(m, C: int) -> bool:
    """``m`` is this module's ``RMSNorm`` over C columns with fp32 weight and bias, the norm the HIP epilogue takes."""
    return (isinstance(m, RMSNorm) and all(isinstance(p, torch.Tensor) and p.dtype == torch.float32
                                           and tuple(p.shape) == (C,) for p in (m.weight, m.bias)))


class DataEmbedding(nn.Module):
    """value Linear(N -> d_model) + positional (+ optional time-feature Linear), with the
    reference's four normalisation modes ("decoupled" = value + gate * LayerNorm(aux))."""

    _VALID_NORM_MODES = {"none", "layer", "rms", "decoupled"}

    def __init__(self, c_in: int, d_model: int, dropout: float, time_features: Optional[int] = None,
                 use_norm: bool = True, embed_norm_mode: Optional[str] = None) -> None:
        super().__init__()
        d_model = int(d_model)
        mode = (embed_norm_mode if embed_norm_mode is not None else ("decoupled" if use_norm else "none")).lower()
        if mode not in self._VALID_NORM_MODES:
            raise ValueError(
                f"embed_norm_mode must be one of {sorted(self._VALID_NORM_MODES)}, got {embed_norm_mode!r}")
        self.embed_norm_mode = mode
        self.use_norm = mode != "none"
        self.value_embedding = nn.Linear(int(c_in), d_model)
        self.position_embedding = PositionalEmbedding(d_model)
        self.temporal_embedding: Optional[nn.Module] = (
            nn.Linear(int(time_features), d_model) if time_features is not None and time_features > 0 else None)
        # exactly one of (aux_norm + gate) / norm / nothing, by mode; `gate` is always a registered name
        self.norm: Optional[nn.Module] = {"layer": lambda: nn.LayerNorm(d_model), "rms": lambda: RMSNorm(d_model)}.get(
            mode, lambda: None)()
        self.aux_norm: Optional[nn.Module] = nn.LayerNorm(d_model) if mode == "decoupled" else None
        if mode == "decoupled":
            self.gate = nn.Parameter(torch.full((1, 1, d_model), 0.1, dtype=torch.float32))
        else:
            self.register_parameter("gate", None)
        self.dropout = nn.Dropout(float(dropout))

    @staticmethod
    def _fold_series(x: torch.Tensor, mark: Optional[torch.Tensor]):
        """[B, L, N, C] input: every series becomes its own sample (the reference's plain reshape, :1290-1309)."""
        B, L, N, C = x.shape
        if mark is not None:
            if mark.ndim == 3:
                if tuple(mark.shape[:2]) != (B, L):
                    raise ValueError("x_mark must match batch/time dimensions of x")
                mark = mark.unsqueeze(2).expand(-1, -1, N, -1)
            elif mark.ndim != 4:
                raise ValueError("x_mark must have shape [B, L, T] or [B, L, N, T]")
            elif tuple(mark.shape[:3]) != (B, L, N):
                raise ValueError("x_mark must align with [B, L, N] dimensions of x")
            mark = mark.reshape(B * N, L, mark.size(-1))
        return x.reshape(B * N, L, C), mark

    def aux_term(self, x: torch.Tensor, mark: Optional[torch.Tensor]) -> torch.Tensor:
        """Everything added to the value embedding: positions (+ time features), gated and normalised in the
        "decoupled" mode.  [1 or B, L, d_model]."""
        aux = self.position_embedding(x)
        if mark is not None and self.temporal_embedding is not None:
            aux = aux + self.temporal_embedding(mark)
        if self.aux_norm is not None:
            aux = self.gate.to(aux.dtype) * _norm(self.aux_norm, aux)
        return aux

    def forward(self, x: torch.Tensor, x_mark: Optional[torch.Tensor] = None) -> torch.Tensor:
        lead = None
        if x.ndim == 4:
            lead = tuple(x.shape[:3])
            x, x_mark = self._fold_series(x, x_mark)
        elif x.ndim != 3:
            raise ValueError("DataEmbedding expects input shaped [B, L, C] or [B, L, N, C]")
        elif x_mark is not None and x_mark.ndim != 3:
            raise ValueError("x_mark must share dimensions [B, L, T]")
        out = self.value_embedding(x) + self.aux_term(x, x_mark)
        if self.norm is not None:
            out = _norm(self.norm, out)
        out = self.dropout(out)
        return out if lead is None else out.view(*lead, out.size(-1))


# -------------------------------------------------------------------------
# TimesNet                                               reference :1374-2102
# -------------------------------------------------------------------------
class _Aux(NamedTuple):
    """The epilogue term of the embedding, not yet formed: ``_through_weight`` writes it and the context terms into
    ``add`` in one pass (``ftn_embed_add``)."""
    mark: Optional[torch.Tensor]
    L: int
    device: torch.device


def _fp32_no_grad(tensors) -> bool:
    """Every tensor is fp32, and nothing asks autograd to follow them (the HIP kernels are forward-only)."""
    tensors = [t for t in tensors if t is not None]
    return all(t.dtype == torch.float32 for t in tensors) and not (
        torch.is_grad_enabled() and any(t.requires_grad for t in tensors))


class _Dims(NamedTuple):
    """What the lazily built layers are sized from (one call's view of the inputs)."""
    n_series: int
    time_dim: int
    static_dim: int
    id_dim: int
    steps: int
    d_model: int

    @property
    def ctx(self) -> int:
        return self.static_dim + self.id_dim


def _zero_linear(i: int, o: int) -> nn.Linear:
    lin = nn.Linear(i, o)
    with torch.no_grad():
        lin.weight.zero_()
        lin.bias.zero_()
    return lin


def _ln_of(width: int) -> Callable[[nn.Module], bool]:
    return lambda m: isinstance(m, nn.LayerNorm) and tuple(m.normalized_shape) == (width,)


def _lin_of(i: int, o: int) -> Callable[[nn.Module], bool]:
    return lambda m: isinstance(m, nn.Linear) and (m.in_features, m.out_features) == (i, o)


class _Lazy(NamedTuple):
    """One lazily built sub-module of TimesNet: attribute name, whether this configuration has it at all, whether an
    existing instance still fits the current sizes, and how to build it.  The state_dict keys (= the attribute names)
    and the initial values (zero heads / zero context maps, reference :1660-1662, :1719-1720, :1825-1842) are the
    checkpoint contract; the order of the table is the order of first construction."""
    name: str
    wanted: Callable[["TimesNet", _Dims], bool]
    fits: Callable[["TimesNet", _Dims], Callable[[nn.Module], bool]]
    make: Callable[["TimesNet", _Dims], nn.Module]


_HAS_CTX = lambda net, d: d.ctx > 0
_LAZY_TABLE: Tuple[_Lazy, ...] = (
    _Lazy("context_norm", _HAS_CTX, lambda net, d: _ln_of(d.ctx), lambda net, d: nn.LayerNorm(d.ctx)),
    _Lazy("context_coeff", lambda net, d: d.ctx > 0 and net.use_zero_mean_context and net.context_rank > 0,
          lambda net, d: _lin_of(d.ctx, net.context_rank), lambda net, d: _zero_linear(d.ctx, net.context_rank)),
    _Lazy("temporal_context", lambda net, d: d.ctx > 0 and net.use_zero_mean_context and net.context_rank > 0,
          lambda net, d: (lambda m: getattr(m, "rank", None) == net.context_rank),
          lambda net, d: LowRankTemporalContext(net.context_rank, net.context_scale_default)),
    _Lazy("context_proj", lambda net, d: d.ctx > 0 and net.use_constant_context_bias,
          lambda net, d: _lin_of(d.ctx, 1), lambda net, d: _zero_linear(d.ctx, 1)),
    _Lazy("late_bias_norm", lambda net, d: d.ctx > 0 and net.use_late_bias_head,
          lambda net, d: _ln_of(d.ctx), lambda net, d: nn.LayerNorm(d.ctx)),
    _Lazy("late_bias_head", lambda net, d: d.ctx > 0 and net.use_late_bias_head,
          lambda net, d: _lin_of(d.ctx, d.steps), lambda net, d: _zero_linear(d.ctx, d.steps)),
    # built for checkpoint compatibility only: the reference never applies it in forward (:1754-1774)
    _Lazy("pre_embedding_norm", lambda net, d: True,
          lambda net, d: ((lambda m: isinstance(m, nn.Identity)) if d.ctx == 0 else _ln_of(1 + d.ctx)),
          lambda net, d: nn.Identity() if d.ctx == 0 else nn.LayerNorm(1 + d.ctx)),
    _Lazy("embedding", lambda net, d: True, lambda net, d: (lambda m: True),
          lambda net, d: DataEmbedding(d.n_series, d.d_model, net.dropout, time_features=d.time_dim or None,
                                       use_norm=net.use_embedding_norm, embed_norm_mode=net.embed_norm_mode)),
    _Lazy("layer_norm", lambda net, d: True, lambda net, d: _ln_of(d.d_model), lambda net, d: nn.LayerNorm(d.d_model)),
    _Lazy("mu_head", lambda net, d: True, lambda net, d: _lin_of(d.d_model, d.n_series),
          lambda net, d: _zero_linear(d.d_model, d.n_series)),
    _Lazy("sigma_head", lambda net, d: True, lambda net, d: _lin_of(d.d_model, d.n_series),
          lambda net, d: _zero_linear(d.d_model, d.n_series)),
)


class TimesNet(nn.Module):
    """Embedding -> n_layers x (TimesBlock, residual, shared LayerNorm) -> time projection
    L -> H -> rate / dispersion heads (negative-binomial parameters)."""

    def __init__(self, input_len: int, pred_len: int, d_model: int, n_layers: int, k_periods: int,
                 kernel_set, dropout: float, activation: str, mode: str, d_ff: Optional[int] = None,
                 bottleneck_ratio: float = 1.0, min_period_threshold: int = 1, channels_last: bool = False,
                 use_checkpoint: bool = True, use_embedding_norm: bool = True,
                 embed_norm_mode: Optional[str] = None, min_sigma: float = 1e-3,
                 min_sigma_vector=None, id_embed_dim: int = 32, static_proj_dim: Optional[int] = None,
                 static_layernorm: bool = True, use_zero_mean_context: bool = False, context_rank: int = 0,
                 context_scale: float = 1e-2, use_constant_context_bias: bool = False,
                 use_late_bias_head: bool = True) -> None:
        super().__init__()
        del channels_last                      # accepted for signature compatibility only
        assert mode in ("direct", "recursive")
        # -- validated scalars
        checks = ((d_ff is None or int(d_ff) > 0, "d_ff must be a positive integer"),
                  (float(bottleneck_ratio) > 0, "bottleneck_ratio must be a positive value"),
                  (int(id_embed_dim) >= 0, "id_embed_dim must be non-negative"),
                  (static_proj_dim is None or int(static_proj_dim) > 0,
                   "static_proj_dim must be a positive integer when provided"),
                  (int(context_rank) >= 0, "context_rank must be non-negative"))
        for ok, msg in checks:
            if not ok:
                raise ValueError(msg)
        self.mode = mode
        self.input_len, self.pred_len = int(input_len), int(pred_len)
        self.requested_d_model = int(d_model)
        self.requested_d_ff = None if d_ff is None else int(d_ff)
        self.d_model: Optional[int] = None
        self.d_ff: Optional[int] = self.requested_d_ff
        self.bottleneck_ratio = float(bottleneck_ratio)
        self.n_layers, self.dropout = int(n_layers), float(dropout)
        self.use_checkpoint = bool(use_checkpoint)
        self.use_embedding_norm = bool(use_embedding_norm)
        self.embed_norm_mode = embed_norm_mode or ("decoupled" if self.use_embedding_norm else "none")
        self.min_sigma = float(min_sigma)
        self.k_periods = int(k_periods)
        self.kernel_set = list(kernel_set)
        self.id_embed_dim = int(id_embed_dim)
        self.static_proj_dim = None if static_proj_dim is None else int(static_proj_dim)
        self.static_layernorm = bool(static_layernorm)
        self.use_zero_mean_context = bool(use_zero_mean_context)
        self.use_constant_context_bias = bool(use_constant_context_bias)
        self.use_late_bias_head = bool(use_late_bias_head)
        self.context_rank = int(context_rank)
        self.context_scale_default = float(context_scale)
        self.debug_memory = False
        self._out_steps = self.pred_len if mode == "direct" else 1

        # -- modules that exist from the start
        self.period_selector = FFTPeriodSelector(self.k_periods, self.input_len, min_period_threshold)
        self.blocks = nn.ModuleList(
            TimesBlock(None, self.kernel_set, self.dropout, activation, d_ff=self.requested_d_ff,
                       bottleneck_ratio=self.bottleneck_ratio) for _ in range(self.n_layers))
        for depth, blk in enumerate(self.blocks):
            blk.block_index = depth
            object.__setattr__(blk, "period_selector", self.period_selector)   # shared, registered once
        self.residual_dropout = nn.Dropout(self.dropout)
        self.pre_embedding_dropout = nn.Dropout(self.dropout)
        # the time projection starts as "repeat the last observed step" (:1451-1455)
        self.forecast_time_proj = _zero_linear(self.input_len, self.pred_len)
        if self.pred_len > 0:
            with torch.no_grad():
                self.forecast_time_proj.weight[:, -1].fill_(1.0)

        # -- everything below is built on the first forward (reference :1514-1849); None until then
        for name in ("layer_norm", "embedding", "mu_head", "sigma_head", "series_embedding", "static_proj",
                     "static_norm", "context_norm", "context_proj", "context_coeff", "temporal_context",
                     "late_bias_norm", "late_bias_head", "pre_embedding_norm"):
            setattr(self, name, None)
        self.register_parameter("late_bias_gate", None)
        self.register_buffer("min_sigma_vector", None)
        if min_sigma_vector is not None:
            self.min_sigma_vector = torch.as_tensor(min_sigma_vector, dtype=torch.float32).reshape(1, 1, -1)
        self.embedding_time_features: Optional[int] = None
        self.output_dim: Optional[int] = None
        self.input_channels: Optional[int] = None
        self._static_in_features: Optional[int] = None
        self._static_out_dim = 0
        self._series_id_vocab: Optional[int] = None
        self._series_id_reference: Optional[torch.Tensor] = None
        self._last_head_backend = "torch"
        self._last_timeproj_backend = "torch"
        self._last_embed_backend = "torch"
        self._last_context_backend = "torch"       # "hip": every piece of the last context front end ran in HIP
        self._ctx_rows_torch = False
        self._defer_checks = False
        self._pending_bad = None

    # ---- lazy construction ------------------------------------------------------
    def _bind_static(self, series_static: Optional[torch.Tensor], n_series: int, ref: torch.Tensor) -> int:
        """Static covariates -> ``static_proj`` (+ ``static_norm``); returns the projected width (0 = unused)."""
        if series_static is not None:
            if series_static.ndim not in (2, 3):
                raise ValueError("series_static must have shape [N, F] or [B, N, F]")
            rows, feat = series_static.shape[-2], int(series_static.shape[-1])
            if rows != n_series:
                raise ValueError("series_static must align with the number of input series")
            if feat <= 0:
                raise ValueError("series_static must have at least one feature")
            if self.static_proj is None:
                width = feat if self.static_proj_dim is None else self.static_proj_dim
                self.static_proj = nn.Linear(feat, width)
                self.static_norm = nn.LayerNorm(width) if self.static_layernorm else nn.Identity()
                self._static_in_features = feat
            elif self.static_proj.in_features != feat:
                raise ValueError("series_static feature dimension changed between calls")
        if self.static_proj is None:
            return 0
        self.static_proj = _place(self.static_proj, ref)
        if self.static_norm is not None:
            self.static_norm = _place(self.static_norm, ref)
        return int(self.static_proj.out_features)

    def _bind_ids(self, series_ids: Optional[torch.Tensor], n_series: int, ref: torch.Tensor) -> int:
        """Series identifiers -> ``series_embedding`` and the remembered id row; returns the embedding width."""
        if self.id_embed_dim <= 0:
            return 0
        row = None
        if series_ids is not None:
            if series_ids.ndim not in (1, 2):
                raise ValueError("series_ids must have shape [N] or [B, N]")
            row = (series_ids if series_ids.ndim == 1 else series_ids[0]).to(torch.long)
            if row.numel() != n_series:
                raise ValueError("series_ids length must match number of series")
        vocab = (lambda t: int(t.max().item()) + 1 if t.numel() else n_series)
        if self.series_embedding is None:
            if row is None:
                row = torch.arange(n_series, dtype=torch.long, device=ref.device)
            self.series_embedding = nn.Embedding(vocab(row), self.id_embed_dim)
        elif row is not None and not self._defer_checks and vocab(row) > int(self.series_embedding.num_embeddings):
            raise ValueError("series_ids vocabulary expanded between calls")     # (one host read; skipped in a capture)
        self.series_embedding = _place(self.series_embedding, ref)
        if row is not None:
            self._series_id_reference = row.to(ref.device)
        elif self._series_id_reference is None:
            self._series_id_reference = torch.arange(n_series, dtype=torch.long, device=ref.device)
        if self._series_id_reference.numel() != n_series:
            raise ValueError("series identifier count changed between calls")
        self._series_id_vocab = int(self.series_embedding.num_embeddings)
        return int(self.series_embedding.embedding_dim)

    def _ensure_embedding(self, x, x_mark=None, series_static=None, series_ids=None) -> None:
        """Build / resize / move every lazily constructed layer for this call's input sizes (:1514-1849)."""
        n_series, time_dim = x.shape[-1], (0 if x_mark is None else x_mark.shape[-1])
        for attr, val, msg in (("input_channels", n_series, "Number of series changed between calls"),
                               ("d_model", self.requested_d_model, "d_model changed between calls")):
            have = getattr(self, attr)
            if have is not None and have != val:
                raise ValueError(msg)
            setattr(self, attr, val)
        if self.embedding_time_features not in (None, time_dim):
            raise ValueError("Temporal feature dimension changed between calls")
        self.d_ff = self.requested_d_ff if self.requested_d_ff is not None else self.d_model
        self._static_out_dim = self._bind_static(series_static, n_series, x)
        dims = _Dims(n_series, time_dim, self._static_out_dim, self._bind_ids(series_ids, n_series, x),
                     self._out_steps, self.d_model)

        for spec in _LAZY_TABLE:
            mod = getattr(self, spec.name)
            if not spec.wanted(self, dims):
                mod = None
            else:
                if mod is None or not spec.fits(self, dims)(mod):
                    mod = spec.make(self, dims)
                mod = _place(mod, x)
            setattr(self, spec.name, mod)
        # the late-bias gate is a bare Parameter next to its head (:1836-1847)
        if self.late_bias_head is None:
            self.late_bias_gate = None
        else:
            gate, want = self.late_bias_gate, (1, dims.steps, 1)
            if isinstance(gate, nn.Parameter) and tuple(gate.shape) == want:
                gate.data = gate.data.to(x.device, torch.float32)
            else:
                self.late_bias_gate = nn.Parameter(torch.full(want, 0.05, device=x.device))
        self.pre_embedding_dropout.to(x.device)
        self.forecast_time_proj = _place(self.forecast_time_proj, x)

        floor = self._floor_vector()
        if floor is not None:
            if int(floor.shape[-1]) < n_series:
                raise ValueError("min_sigma_vector length does not match number of series")
            self.min_sigma_vector = floor[..., :n_series]
        self.embedding_time_features = time_dim
        self.output_dim = n_series

    def _floor_vector(self) -> Optional[torch.Tensor]:
        """``min_sigma_vector`` when it is set (any shape, N elements), else None: the scalar ``min_sigma`` applies."""
        floor = self.min_sigma_vector
        return floor if isinstance(floor, torch.Tensor) and floor.numel() > 0 else None

    def _uses_ids(self) -> bool:
        return self.series_embedding is not None and self.id_embed_dim > 0

    # ---- series context: [Bc, N, ctx] rows the context / late-bias maps read ----------------
    def _context_rows(self, window, series_static, series_ids) -> Optional[torch.Tensor]:
        """``_rows_of`` for the whole model: missing ids default to the remembered ones, given ids are remembered."""
        B, _, N = window.shape
        if (self.static_proj is not None and series_static is not None and series_static.ndim == 3
                and series_static.size(0) != B):
            raise ValueError("series_static batch dimension must match input batch size")
        ids = series_ids
        if self._uses_ids():
            if series_ids is not None:
                ids = series_ids.view(1, -1) if series_ids.ndim == 1 else series_ids
                if ids.size(0) not in (1, B):
                    raise ValueError("series_ids batch dimension does not match input")
                if ids.size(1) != N:
                    raise ValueError("series_ids length must match number of series")
                ids = ids.to(device=window.device, dtype=torch.long)
                self._series_id_reference = ids[0].detach().clone()
            else:
                remembered = self._series_id_reference
                if remembered is not None and remembered.numel() != N:
                    raise ValueError("Stored series identifiers do not match input dimension")
                ids = (torch.arange(N, device=window.device) if remembered is None else remembered.to(window.device)).view(1, N)
        return self._rows_of(window, series_static, ids)

    def _rows_of(self, window, static, ids) -> Optional[torch.Tensor]:
        """Static projection and id embedding side by side, through ``context_norm`` (:1883-1956), from checked
        inputs: ``static`` None, [N, F] or [B, N, F]; ``ids`` long [1|B, N] on the window's device when the model
        embeds ids (otherwise only their batch shape is looked at).  Every op is row-wise, so when the static
        features / ids are shared by the batch (2-D / one-row inputs, the pipeline's case) the rows are built once
        (Bc = 1) and broadcast by their consumers."""
        B = window.size(0)
        shared = (static is None or static.ndim == 2) and (ids is None or ids.ndim == 1 or ids.size(0) == 1)
        Bc = 1 if shared else B
        if self._hip_rows_ok(window, static):
            return self._rows_hip(window, static, ids, Bc)
        self._last_context_backend = "torch"
        self._ctx_rows_torch = False
        cols = []
        if self.static_proj is not None and static is not None:
            st = static if static.ndim == 3 else static.unsqueeze(0).expand(Bc, -1, -1)
            proj = self.static_proj(st.to(device=window.device, dtype=window.dtype, non_blocking=window.is_cuda))
            cols.append(proj if self.static_norm is None else _norm(self.static_norm, proj))
        if self._uses_ids():
            cols.append(self.series_embedding(ids.expand(Bc, -1) if ids.size(0) != Bc else ids))
        if not cols:
            return None
        self._ctx_rows_torch = True
        rows = cols[0] if len(cols) == 1 else torch.cat(cols, dim=-1)
        return rows if self.context_norm is None else _norm(self.context_norm, rows)

    def _row_heads(self):
        """Which maps of the series rows this model applies: ``(coefficients, constant bias, late bias)``."""
        return (self.context_coeff is not None and self.temporal_context is not None and self.use_zero_mean_context,
                self.context_proj is not None and self.use_constant_context_bias,
                self.late_bias_head is not None and self.late_bias_norm is not None
                and isinstance(self.late_bias_gate, nn.Parameter))

    def _hip_rows_ok(self, window, static) -> bool:
        """``ftn_context_rows`` takes this model's rows: ROCm fp32 tensors, no autograd, affine LayerNorms, sizes
        inside the kernel's limits."""
        if not (_CTX_HIP and window.is_cuda and window.dtype == torch.float32):
            return False
        use_static = self.static_proj is not None and static is not None
        if not (use_static or self._uses_ids()) or not _affine_layernorm(self.context_norm, self._ctx_width(use_static)):
            return False
        has_coeff, has_bias, has_late = self._row_heads()
        mods = [self.context_norm, self.context_coeff if has_coeff else None, self.context_proj if has_bias else None]
        tensors = [self.late_bias_gate] if has_late else []
        if use_static:
            sn, sp = self.static_norm, self.static_proj
            if not (sn is None or isinstance(sn, nn.Identity) or _affine_layernorm(sn, sp.out_features)):
                return False
            if max(sp.in_features, sp.out_features) > _CTX_MAX:
                return False
            mods += [sp, None if isinstance(sn, nn.Identity) else sn]
            tensors.append(static)
        if self._uses_ids():
            mods.append(self.series_embedding)
        if has_coeff and self.context_coeff.out_features > _CTX_RMAX:
            return False
        if has_late:
            if not _affine_layernorm(self.late_bias_norm, self.context_norm.normalized_shape[0]):
                return False
            mods += [self.late_bias_norm, self.late_bias_head]
        tensors += [p for m in mods if m is not None for p in m.parameters()]
        return self.context_norm.normalized_shape[0] <= _CTX_MAX and _fp32_no_grad(tensors)

    def _ctx_width(self, use_static: bool) -> int:
        return ((self.static_proj.out_features if use_static else 0)
                + (self.series_embedding.embedding_dim if self._uses_ids() else 0))

    def _rows_hip(self, window, static, ids, Bc: int) -> torch.Tensor:
        """The HIP body of ``_rows_of``: one launch gives the rows and every map of them this model applies; the rows
        carry the maps' results (``_ftn_ctx``), which ``_context_terms`` and ``_late_bias`` hand back."""
        from .. import runtime

        has_coeff, has_bias, has_late = self._row_heads()
        lin = lambda m: (m.weight, m.bias)
        kw = {}
        if self.static_proj is not None and static is not None:
            sn = self.static_norm
            kw.update(static=static.to(device=window.device, non_blocking=True), static_proj=lin(self.static_proj),
                      static_norm=None if sn is None or isinstance(sn, nn.Identity) else _ln_params(sn))
        if self._uses_ids():
            kw.update(ids=ids, table=self.series_embedding.weight)
        rows, coeff, cbias, late = runtime.context_rows(
            Bc, window.size(2), _ln_params(self.context_norm),
            coeff=lin(self.context_coeff) if has_coeff else None, proj=lin(self.context_proj) if has_bias else None,
            late=((_ln_params(self.late_bias_norm),) + lin(self.late_bias_head) + (self.late_bias_gate.reshape(-1),)
                  if has_late else None), **kw)
        rows._ftn_ctx = (coeff, cbias, late)
        self._last_context_backend = "hip"
        self._ctx_rows_torch = False
        return rows

    # ---- embedding front end ---------------------------------------------------------------
    def _hip_embed_ok(self, window: torch.Tensor) -> bool:
        emb = self.embedding
        if emb is None or emb.embed_norm_mode not in ("decoupled", "none", "layer", "rms"):
            return False
        if emb.embed_norm_mode == "rms" and not _affine_rmsnorm(emb.norm, self.d_model):
            return False
        if emb.embed_norm_mode == "layer" and not (isinstance(emb.norm, nn.LayerNorm) and emb.norm.weight is not None
                                                   and emb.norm.bias is not None):
            return False
        return (window.is_cuda and window.dtype == torch.float32
                and not (torch.is_grad_enabled() and (window.requires_grad or emb.value_embedding.weight.requires_grad))
                and not (self.training and self.dropout > 0.0) and hip_shell_width_ok(self.d_model)
                and window.stride(2) == 1 and window.stride(1) == window.size(2))

    def _context_terms(self, rows):
        """The temporal-context coefficients and the constant context bias of the series rows (None when unused)."""
        coeff = bias = None
        if rows is not None and getattr(rows, "_ftn_ctx", None) is not None:
            return rows._ftn_ctx[:2]
        if rows is not None:
            if self.context_coeff is not None and self.temporal_context is not None and self.use_zero_mean_context:
                coeff = self.context_coeff(rows.to(self.context_coeff.weight.dtype))
            if self.context_proj is not None and self.use_constant_context_bias:
                bias = self.context_proj(rows.to(self.context_proj.weight.dtype)).squeeze(-1)
        return coeff, bias

    def _through_weight(self, add, coeff, bias, L: int, w):
        """``add`` (None = nothing yet) plus the two context terms pushed through the value weight ``w`` [D, N] (or a
        column slice of it): ``(add + project(coeff)) + bias @ w^T``, summed left to right - the recursive forecaster
        and the graph tests rest on these bits.  None when there is nothing to add.  ``add`` may be the epilogue term
        not yet formed (``_Aux``): the HIP body forms it and adds the context terms in one pass (``ftn_embed_add``)."""
        if isinstance(add, _Aux) or (add is None and self._hip_terms_ok(coeff, bias, w)):
            return self._hip_add(add, coeff, bias, L, w)
        terms = (None if coeff is None else self.temporal_context.project(coeff.detach().float(), L, w),
                 None if bias is None else (bias.detach().float() @ w.t()).unsqueeze(1))
        for term in terms:
            if term is not None:
                add = term if add is None else add + term
        return add

    def _embed_epilogue(self, window, mark, defer: bool = False):
        """What is added to ``x W^T`` once, whatever the series: value bias + positional (+ time-feature) term, gated
        and normalised in the "decoupled" mode, ``[1|B, L, D]``; and ``(gamma, beta, eps)`` of the "layer" mode's
        LayerNorm or ``(gamma, beta, eps, "rms")`` of the "rms" mode's norm (None otherwise).  ``defer``: on the HIP
        path the term comes back unformed (``_Aux``), for ``_through_weight`` to write together with the context
        terms."""
        emb = self.embedding
        ln = _ln_params(emb.norm) if emb.embed_norm_mode == "layer" else None
        if emb.embed_norm_mode == "rms":
            ln = _ln_params(emb.norm) + ("rms",)
        if self._hip_epilogue_ok(window, mark):
            aux = _Aux(mark if emb.temporal_embedding is not None else None, window.size(1), window.device)
            return (aux if defer else self._hip_add(aux, None, None, aux.L, None)), ln
        self._last_context_backend = "torch"
        add = emb.aux_term(window[:1], mark) + emb.value_embedding.bias.detach()
        return add, ln

    def _hip_epilogue_ok(self, window, mark) -> bool:
        """``ftn_embed_add`` forms this embedding's epilogue term."""
        emb = self.embedding
        if not (_CTX_HIP and window.is_cuda and window.dtype == torch.float32 and hip_shell_width_ok(self.d_model)
                and emb.embed_norm_mode in ("none", "decoupled", "layer", "rms")):
            return False
        if emb.embed_norm_mode == "rms" and not _affine_rmsnorm(emb.norm, self.d_model):
            return False
        mods = [emb.value_embedding]
        tensors = []
        if mark is not None and emb.temporal_embedding is not None:
            if not (isinstance(emb.temporal_embedding, nn.Linear) and mark.ndim == 3 and mark.is_cuda
                    and emb.temporal_embedding.in_features <= _ADD_TMAX):
                return False
            mods.append(emb.temporal_embedding)
            tensors.append(mark)
        if emb.aux_norm is not None:
            if not _affine_layernorm(emb.aux_norm, self.d_model) or emb.gate is None:
                return False
            mods.append(emb.aux_norm)
            tensors.append(emb.gate)
        return _fp32_no_grad(tensors + [p for m in mods for p in m.parameters()])

    def _hip_terms_ok(self, coeff, bias, w) -> bool:
        """``ftn_context_through_weight`` + ``ftn_embed_add`` take these context terms and this weight."""
        if not (_CTX_HIP and (coeff is not None or bias is not None) and w.is_cuda and w.ndim == 2
                and w.size(0) % 4 == 0 and w.size(0) <= 512):
            return False
        if coeff is not None and not (coeff.ndim == 3 and coeff.size(2) <= _CTX_RMAX
                                      and self.temporal_context is not None):
            return False
        scale = None if coeff is None else self.temporal_context.scale
        return all(t is None or t.is_cuda for t in (coeff, bias)) and _fp32_no_grad([coeff, bias, w, scale])

    def _hip_add(self, aux, coeff, bias, L: int, w) -> torch.Tensor:
        """The HIP body of ``_embed_epilogue`` + ``_through_weight``: the context terms through ``w``
        (``ftn_context_through_weight``, kept with the terms for the later steps of a recursive forecast), then
        ``add`` in one pass.  Terms the kernels do not take (``_hip_terms_ok``) are added by the torch composition."""
        from .. import runtime

        emb = self.embedding
        q_coeff = q_bias = None
        terms_hip = (coeff is not None or bias is not None) and self._hip_terms_ok(coeff, bias, w)
        if terms_hip:
            holder = coeff if coeff is not None else bias
            key = (tuple(w.shape), w.stride(0)) + _param_key((w,))
            kept = getattr(holder, "_ftn_q", None)
            if kept is None or kept[0] != key:
                kept = (key,) + runtime.context_through_weight(coeff, bias, w)
                holder._ftn_q = kept
            q_coeff, q_bias = kept[1], kept[2]
        kw = {}
        device = aux.device if aux is not None else w.device
        D = self.d_model if aux is not None else w.size(0)
        if aux is not None:
            kw.update(pos=emb.position_embedding.table(L, device), b_v=emb.value_embedding.bias, mark=aux.mark)
            if aux.mark is not None:
                kw.update(time=(emb.temporal_embedding.weight, emb.temporal_embedding.bias))
            if emb.aux_norm is not None:
                kw.update(aux=_ln_params(emb.aux_norm) + (emb.gate.reshape(-1),))
        if q_coeff is not None:
            tc = self.temporal_context
            tc._last_backend = "fused"
            kw.update(basisc=self._centred_basis(L, q_coeff), scale=tc.scale.reshape(1))
        add = runtime.embed_add(L, D, device, q_coeff=q_coeff, q_bias=q_bias, **kw)
        self._last_context_backend = "torch" if self._ctx_rows_torch else "hip"
        if not terms_hip and (coeff is not None or bias is not None):
            self._last_context_backend = "torch"
            add = self._through_weight(add, coeff, bias, L, w)
        return add

    def _centred_basis(self, L: int, ref: torch.Tensor) -> torch.Tensor:
        """The doubly centred DCT basis of ``LowRankTemporalContext.project`` [L, R]: a function of (L, rank, device),
        kept between calls."""
        tc = self.temporal_context
        key = (L, tc.rank, str(ref.device))
        kept = self.__dict__.get("_basisc")
        if kept is None or kept[0] != key:
            basis = tc._basis(L, ref)
            kept = (key, (basis - basis.mean(dim=0, keepdim=True)).float().contiguous())
            self.__dict__["_basisc"] = kept
        return kept[1]

    def _hip_embed_terms(self, window, mark, coeff, bias):
        """What the HIP embedding adds to ``x W^T``: ``(w, add, ln)`` with ``w`` the value weight [D, N], ``add`` the
        epilogue term + the two context terms pushed through ``w``, contiguous fp32 ``[1|B, L, D]``, and ``ln`` of
        ``_embed_epilogue``.  Shared by ``_embed`` and the recursive forecaster (``forecast.py``), which embeds its
        window row by row."""
        w = self.embedding.value_embedding.weight.detach()
        add, ln = self._embed_epilogue(window, mark, defer=True)
        add = self._through_weight(add, coeff, bias, window.size(1), w)
        return w, add.detach().float().contiguous(), ln

    def _with_context(self, window, coeff, bias) -> torch.Tensor:
        """``window + temporal context + constant bias`` as a [B, L, N] tensor (the torch path of the embedding)."""
        feats = window
        if coeff is not None:
            signal = self.temporal_context(coeff, window.size(1))          # HIP LRTC kernel on ROCm tensors
            if signal.ndim != 3 or signal.shape[1:] != window.shape[1:] or signal.size(0) not in (1, window.size(0)):
                raise RuntimeError("Temporal context must align with the [B, L, N] input")
            feats = feats + signal.to(feats.dtype)
        if bias is not None:
            feats = feats + bias.to(feats.dtype).unsqueeze(1)
        return feats

    def _embed(self, window, mark, rows) -> torch.Tensor:
        """``embedding(window + temporal context + constant bias)`` (:1958-2020).  On the HIP path the two context
        terms are pushed through the value embedding's weight instead (``x W^T + (basis coeff^T + cb) W^T``): one pass
        over the window (``ftn_embed_forward``) and the [B, L, N] context tensor is never formed."""
        coeff, bias = self._context_terms(rows)
        if self._hip_embed_ok(window):
            from .. import runtime

            w, add, ln = self._hip_embed_terms(window, mark, coeff, bias)
            self._last_embed_backend = "hip"
            seq = runtime.embed_forward(window, w, add, ln)
        else:
            seq = self.embedding(self._with_context(window, coeff, bias), mark)
        if seq.ndim != 3 or seq.size(1) != self.input_len or seq.size(-1) != self.d_model:
            raise RuntimeError("Embedding output must have shape [B, input_len, d_model]")
        return seq

    # ---- block stack: x <- LayerNorm(x + dropout(block(x) - x)), one shared LayerNorm (:2022-2061) --------------
    def _stack(self, seq: torch.Tensor) -> torch.Tensor:
        self.period_selector = self.period_selector.to(device=seq.device, dtype=seq.dtype)
        for blk in self.blocks:
            object.__setattr__(blk, "period_selector", self.period_selector)
        recompute = self.use_checkpoint and torch.is_grad_enabled()
        plain_eval = not recompute and not (self.training and self.dropout > 0.0)
        for blk in self.blocks:
            if plain_eval:       # dropout is the identity: residual + LayerNorm ride in the block's last kernel
                seq = blk(seq, post_norm=self.layer_norm)
            else:
                new = checkpoint(blk, seq, use_reentrant=False) if recompute else blk(seq)
                seq = _norm(self.layer_norm, seq + self.residual_dropout(new - seq))
        return seq

    # ---- heads -----------------------------------------------------------------------------------
    def _hip_heads_ok(self, seq: torch.Tensor, window: torch.Tensor) -> bool:
        params = (self.forecast_time_proj.weight, self.mu_head.weight, self.sigma_head.weight)
        return (seq.is_cuda and seq.dtype == torch.float32 and window.dtype == torch.float32
                and not (torch.is_grad_enabled() and (seq.requires_grad or any(p.requires_grad for p in params)))
                and hip_shell_width_ok(self.d_model)
                and window.stride(2) == 1 and window.stride(1) == window.size(2))

    def _late_bias(self, rows) -> Optional[torch.Tensor]:
        """The gated late-bias head of the series rows, ``[Bc, steps, N]`` (None when the model has none)."""
        if rows is not None and getattr(rows, "_ftn_ctx", None) is not None:
            return rows._ftn_ctx[2]
        if (rows is None or self.late_bias_head is None or self.late_bias_norm is None
                or not isinstance(self.late_bias_gate, nn.Parameter)):
            return None
        head = self.late_bias_head
        lb = head(_norm(self.late_bias_norm, rows.to(device=head.weight.device, dtype=head.weight.dtype)))
        return self.late_bias_gate.to(lb) * lb.transpose(1, 2)

    def _time_projection(self, seq, steps: int, hip: bool) -> torch.Tensor:
        """``forecast_time_proj`` L -> steps (its last ``steps`` rows), ``[B, steps, d_model]``: ``hip`` runs
        ``ftn_timeproj_forward`` straight into that layout (no permute copies)."""
        wt, bt = self.forecast_time_proj.weight, self.forecast_time_proj.bias
        if steps != self.pred_len:
            wt, bt = wt[-steps:], bt[-steps:]
        self._last_timeproj_backend = "hip" if hip else "torch"
        if hip:
            from .. import runtime

            return runtime.timeproj_forward(seq.detach().contiguous(), wt.detach(), bt.detach())
        return torch.matmul(wt, seq) + bt.view(1, -1, 1)

    def _rate_dispersion(self, hidden, window, late, steps: int, heads, hip: bool):
        """``rate = softplus(mu + last observed values (+ late bias)) + 1e-6`` and ``dispersion = softplus(sigma) +
        floor + 1e-6`` (:2063-2102) of ``hidden [B, steps, D]`` for the series of ``heads = (w_mu, b_mu, w_sigma,
        b_sigma, floor vector or None)``: ``(rate, dispersion, bad)`` with ``bad`` the HIP head's device flag (None on
        the torch path, which raises itself).  The torch path applies the weights with ``F.linear``, not through
        ``mu_head`` / ``sigma_head`` as modules: forward hooks on the heads do not run."""
        w_mu, b_mu, w_sigma, b_sigma, floor = heads
        hist = min(steps, window.size(1))
        last = window[:, -hist:, :]
        if hip:
            from .. import runtime

            if floor is not None:
                floor = floor.to(device=hidden.device, dtype=torch.float32).reshape(-1).contiguous()
            return runtime.head_forward(hidden.contiguous(), w_mu.detach(), b_mu.detach(), w_sigma.detach(),
                                        b_sigma.detach(), last, hist,
                                        None if late is None else late.detach().float().contiguous(), floor,
                                        self.min_sigma)
        if hist < steps:                                       # recursive mode / short windows: repeat the last step
            last = torch.cat([last, last[:, -1:, :].expand(-1, steps - hist, -1)], dim=1)
        pre = F.linear(hidden, w_mu, b_mu) + last.to(window.dtype)
        if late is not None:
            pre = pre + late.to(pre.dtype)
        soft = lambda t: F.softplus(t.float(), beta=1.0, threshold=20).to(t.dtype)
        rate = soft(pre) + 1e-6
        spread = soft(F.linear(hidden, w_sigma, b_sigma))
        if floor is None:
            floor = torch.full_like(rate, self.min_sigma)
        else:
            floor = floor.to(device=rate.device, dtype=rate.dtype).reshape(1, 1, -1).expand_as(rate)
        dispersion = spread + floor.to(spread.dtype) + 1e-6
        for name, val in (("rate", rate), ("dispersion", dispersion)):
            if not bool((torch.isfinite(val) & (val > 0)).all()):
                raise RuntimeError(f"Predicted {name} must be finite and strictly positive")
        return rate, dispersion, None

    def _heads(self, seq, window, rows, steps: int):
        """Late bias, time projection L -> steps, then the rate / dispersion heads of every series."""
        B, _, N = window.shape
        late = self._late_bias(rows)
        hip = self._hip_heads_ok(seq, window)
        hidden = self._time_projection(seq, steps, hip)
        heads = (self.mu_head.weight, self.mu_head.bias, self.sigma_head.weight, self.sigma_head.bias,
                 self._floor_vector())
        rate, dispersion, bad = self._rate_dispersion(hidden, window, late, steps, heads, hip)
        if hip:
            self._last_head_backend = "hip"
            # the forward's one synchronisation (range_guard.tripped then reads the blocks' pinned words behind it);
            # deferred, check_outputs() reads the device word after a replay
            self._pending_bad = bad if self._defer_checks else bad.cpu()
        elif rate.shape != (B, steps, N) or dispersion.shape != (B, steps, N):
            raise RuntimeError("Predicted rate/dispersion have incorrect shape")
        return rate, dispersion

    def check_outputs(self) -> None:
        """Raise the reference's RuntimeError (:2095-2098) if the last HIP head call produced a rate or
        dispersion that is not finite and > 0.  Reads one int32 from the device (synchronises); called by
        ``forward`` itself unless ``_defer_checks`` is set (HIP-graph capture, ``graph.GraphedForward``).  Before that,
        a block whose f16x2 range flag tripped inside a captured forward raises ``FloatingPointError``
        (``TimesBlock.check_range``; an eager forward has already repeated itself on bf16x3)."""
        for blk in self.blocks:
            blk.check_range()
        bad, self._pending_bad = self._pending_bad, None
        if bad is None:
            return
        flag = int(bad.item())
        for bit, name in ((1, "rate"), (2, "dispersion")):
            if flag & bit:
                raise RuntimeError(f"Predicted {name} must be finite and strictly positive")

    # ---- series-sharded entry points (dist.SeriesShardedTimesNet): this rank owns series [offset, offset + n) -----
    # Only the value embedding mixes series (a contraction over N); everything else is per series, so a rank computes
    # a partial embedding over its own series, the partials are summed across ranks, and the heads run on the rank's
    # own rows of mu_head / sigma_head.  Each is the stage body above on the rank's slices; none changes the model's
    # state.
    def series_slices(self, offset: int, n: int, device: torch.device) -> dict:
        """This rank's weight slices: ``value_embedding.weight[:, S]`` and the ``heads`` tuple of
        ``_rate_dispersion`` (``mu_head`` / ``sigma_head`` rows, ``min_sigma_vector[S]``).  Cached and keyed on the
        parameters (``_param_key``, as TimesBlock's pack cache)."""
        w_emb, floor = self.embedding.value_embedding.weight, self._floor_vector()
        params = (self.mu_head.weight, self.mu_head.bias, self.sigma_head.weight, self.sigma_head.bias)
        key = (int(offset), int(n), str(device)) + _param_key((w_emb,) + params + (() if floor is None else (floor,)))
        cache = self.__dict__.get("_series_slice_cache")
        if cache is not None and cache[0] == key:
            return cache[1]
        sl = slice(int(offset), int(offset) + int(n))
        own = lambda t: t.to(device=device, dtype=torch.float32).contiguous()
        heads = tuple(own(p.detach()[sl]) for p in params) + (None if floor is None else own(floor.reshape(-1)[sl]),)
        out = {"w_emb": own(w_emb.detach()[:, sl]), "heads": heads}
        self.__dict__["_series_slice_cache"] = (key, out)
        return out

    def series_context_rows(self, window, series_static, series_ids, offset: int) -> Optional[torch.Tensor]:
        """``_rows_of`` for this rank's series without touching the remembered ids: the static features and ids
        are the rank's slices, and missing ids default to the GLOBAL ``arange(offset, offset + n)``."""
        B, _, N = window.shape
        if self.static_proj is not None and series_static is not None and (
                series_static.shape[-2] != N or (series_static.ndim == 3 and series_static.size(0) != B)):
            raise ValueError("series_static must be [n_local, F] or [B, n_local, F] for this rank's series")
        ids = series_ids
        if self._uses_ids():
            if ids is None:
                ids = torch.arange(int(offset), int(offset) + N, device=window.device)
            ids = ids.view(1, -1) if ids.ndim == 1 else ids
            if ids.size(0) not in (1, B) or ids.size(1) != N:
                raise ValueError("series_ids must be [n_local] or [B, n_local] for this rank's series")
            ids = ids.to(device=window.device, dtype=torch.long)
        return self._rows_of(window, series_static, ids)

    def series_partial_embedding(self, window, rows, w_emb: torch.Tensor) -> torch.Tensor:
        """This rank's share of the value embedding, ``[B, L, D]``: ``x_r W_r^T + (context terms of S_r) W_r^T`` -
        no bias, no positional / time-feature term, no norm (``series_embedding_epilogue``: once, after the sum over
        ranks)."""
        coeff, bias = self._context_terms(rows)
        if window.is_cuda:
            from .. import runtime

            add = self._through_weight(None, coeff, bias, window.size(1), w_emb)
            return runtime.embed_forward(window, w_emb, None if add is None else add.contiguous(), None)
        return F.linear(self._with_context(window, coeff, bias), w_emb.to(window.dtype))

    def series_embedding_epilogue(self, window, mark) -> Tuple[torch.Tensor, Optional[tuple]]:
        """What the summed partials still need: ``_embed_epilogue`` with ``add`` as contiguous fp32.  The norm is the
        "layer" mode's LayerNorm or None: the series-sharded forward applies an RMS norm as a module."""
        add, ln = self._embed_epilogue(window, mark)
        return add.detach().float().contiguous(), (ln if ln is None or len(ln) == 3 else None)

    def series_hidden(self, seq: torch.Tensor, steps: int) -> torch.Tensor:
        """``forecast_time_proj`` of the local rows: ``[B_local, steps, d_model]`` (as ``_heads``)."""
        return self._time_projection(seq, steps, seq.is_cuda and seq.dtype == torch.float32
                                     and hip_shell_width_ok(self.d_model))

    def series_heads(self, hidden, window, rows, sl: dict, steps: int):
        """``(rate, dispersion, bad)`` of this rank's series from the gathered ``hidden [B, steps, D]``."""
        return self._rate_dispersion(hidden, window, self._late_bias(rows), steps, sl["heads"], hidden.is_cuda)

    # ---- forward ------------------------------------------------------------------
    def forward(self, x: torch.Tensor, x_mark: Optional[torch.Tensor] = None,
                series_static: Optional[torch.Tensor] = None,
                series_ids: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        out = range_guard.repeat_on_trip(self.blocks, lambda: self._forward_once(x, x_mark, series_static, series_ids),
                                         message="TimesNet: " + range_guard.MESSAGE)
        if not self._defer_checks:
            self.check_outputs()
        return out

    def _forward_once(self, x, x_mark=None, series_static=None, series_ids=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """One pass, without the checks: ``forward`` and the batch-sharded wrapper (``dist.ShardedTimesNet``) decide
        on the f16x2 range around it and call ``check_outputs``."""
        L = self.input_len
        if x.dim() != 3:
            raise ValueError("TimesNet expects input shaped [B, T, N]")
        if x.size(1) < L:
            raise ValueError(f"Input sequence length {x.size(1)} is shorter than required input_len {L}")
        if x_mark is not None and tuple(x_mark.shape[:2]) != tuple(x.shape[:2]):
            raise ValueError("x_mark must share batch/time dimensions with x")
        window = x.narrow(1, x.size(1) - L, L)                    # the last input_len steps (a view)
        mark = None if x_mark is None else x_mark.narrow(1, x_mark.size(1) - L, L)
        self._ensure_embedding(window, mark, series_static, series_ids)
        rows = self._context_rows(window, series_static, series_ids)
        seq = self._stack(self._embed(window, mark, rows))
        return self._heads(seq, window, rows, self._out_steps)

    def head_inputs(self, x: torch.Tensor, x_mark: Optional[torch.Tensor] = None,
                    series_static: Optional[torch.Tensor] = None, series_ids: Optional[torch.Tensor] = None):
        """What the rate / dispersion heads read, for a refit of the heads alone (``fit.refit_heads``): the stage
        bodies of ``forward`` up to ``_time_projection`` under ``no_grad``, so the frozen backbone takes the path an
        inference forward takes even while the head parameters require grad.  Returns ``(hidden, tail, hist, late,
        floor)``: ``hidden [B, steps, d_model]``, ``tail`` the last ``hist`` rows of the input window (a view),
        ``late`` the gated late bias ``[1|B, steps, N]`` or None, ``floor`` ``min_sigma_vector`` flattened or None
        (the scalar ``min_sigma`` applies).  Nothing is recorded for autograd."""
        return self._refit_inputs(x, x_mark, series_static, series_ids, projected=True)

    def output_inputs(self, x: torch.Tensor, x_mark: Optional[torch.Tensor] = None,
                      series_static: Optional[torch.Tensor] = None, series_ids: Optional[torch.Tensor] = None):
        """``head_inputs`` stopped one stage earlier, for a refit of the time projection and the heads
        (``fit.refit_output``): ``(seq, tail, hist, late, floor)`` with ``seq [B, input_len, d_model]`` the block
        stack's output, contiguous, and the rest as ``head_inputs`` returns it.  Nothing is recorded for autograd."""
        return self._refit_inputs(x, x_mark, series_static, series_ids, projected=False)

    def late_rows(self, x: torch.Tensor, x_mark: Optional[torch.Tensor] = None,
                  series_static: Optional[torch.Tensor] = None, series_ids: Optional[torch.Tensor] = None):
        """The frozen series rows the late-bias head reads, for a refit of that head (``fit.late_bias``): what
        ``_refit_inputs`` builds before the embedding - the static projection and the id embedding through
        ``context_norm`` - under ``no_grad``, ``[1|B, N, ctx]`` (one block when the batch shares statics and ids),
        contiguous.  None when the model has no late-bias head.  Nothing is recorded for autograd."""
        with torch.no_grad():
            window, mark = self._refit_window(x, x_mark)
            self._ensure_embedding(window, mark, series_static, series_ids)
            if not self._row_heads()[2]:
                return None
            rows = self._context_rows(window, series_static, series_ids)
            return None if rows is None else rows.detach().contiguous()

    def _refit_window(self, x, x_mark):
        """The last ``input_len`` steps of ``x`` and of ``x_mark`` (views), as every refit entry cuts them."""
        L = self.input_len
        if x.dim() != 3 or x.size(1) < L:
            raise ValueError(f"TimesNet expects input shaped [B, T >= {L}, N]")
        return x.narrow(1, x.size(1) - L, L), None if x_mark is None else x_mark.narrow(1, x_mark.size(1) - L, L)

    def _refit_inputs(self, x, x_mark, series_static, series_ids, projected: bool):
        """The body ``head_inputs`` and ``output_inputs`` share, under ``no_grad`` and the range guard: the first
        leaves after ``_time_projection``, the second before it."""
        def once():
            window, mark = self._refit_window(x, x_mark)
            self._ensure_embedding(window, mark, series_static, series_ids)
            rows = self._context_rows(window, series_static, series_ids)
            seq = self._stack(self._embed(window, mark, rows))
            steps = self._out_steps
            if projected:                                       # hidden [B, steps, D]
                first = self._time_projection(seq, steps, self._hip_heads_ok(seq, window))
            else:                                               # seq [B, L, D]
                first = seq.contiguous()
            hist = min(steps, window.size(1))
            late, floor = self._late_bias(rows), self._floor_vector()
            return (first, window[:, -hist:, :], hist, None if late is None else late.detach(),
                    None if floor is None else floor.detach().reshape(-1))

        with torch.no_grad():
            return range_guard.repeat_on_trip(self.blocks, once, message="TimesNet: " + range_guard.MESSAGE)
