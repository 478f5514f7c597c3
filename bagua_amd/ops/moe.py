"""Index-based ("sparse") MoE token routing.

The dense GShard choreography moves tokens with einsums over a
``(tokens, experts, capacity)`` tensor that is all zeros except ``k``
entries per token. Here the gate emits a :class:`RoutingPlan` of integer
destination rows instead, and rows are copied directly:

* ``assign_slots``  queue position of every token at its chosen expert
  (``cumsum(one_hot) - 1`` gathered at the choice), per-expert counts and
  the inverse map ``src``;
* ``dispatch``      ``(S, M) -> (E*C, M)`` row gather through ``src``;
* ``combine``       ``(E*C, M) -> (S, M)`` weighted sum of ``k`` rows.

Two paths, like the rest of ``bagua_amd.ops``: on GPU with f32/f16/bf16
rows the gfx950 kernels of ``csrc/moe_kernels.hip`` (mandatory there — a
missing extension raises, see ops/native.py); on CPU, or for any other
dtype (float64 gradchecks), an equivalent torch implementation.
"""

from typing import NamedTuple, Optional, Tuple

import torch
from torch import Tensor
from torch.autograd.function import once_differentiable

from . import native

_KERNEL_DTYPES = (torch.float32, torch.float16, torch.bfloat16)


class RoutingPlan(NamedTuple):
    """Where every token goes.

    dest     int32 (k, S): destination row ``expert * capacity + slot``,
             -1 when the choice was dropped or the token is unrouted
    weights  f32 (k, S): combine weight per choice (0 where dropped);
             part of the autograd graph through the gate
    src      int32 (E*C,): token held by each row, -1 for an empty slot
    """

    dest: Tensor
    weights: Tensor
    src: Tensor
    num_experts: int
    capacity: int


def _native_rows(*rows: Tensor) -> bool:
    """True when the row tensors go to the HIP kernels. Raises on a GPU
    machine without the extension rather than falling back."""
    if not all(t.is_cuda for t in rows):
        return False
    if not all(t.dtype in _KERNEL_DTYPES for t in rows):
        return False
    native.require()
    return True


# ---------------------------------------------------------------------------
# slot assignment
# ---------------------------------------------------------------------------

def _assign_slots_torch(expert, num_experts, capacity, base, src):
    S = expert.numel()
    dev = expert.device
    e = expert.long()
    valid = e >= 0
    # stable sort by expert keeps token order inside every queue;
    # unrouted tokens sort behind the last expert
    key = torch.where(valid, e, torch.full_like(e, num_experts))
    skey, order = torch.sort(key, stable=True)
    counts = torch.bincount(key, minlength=num_experts + 1)[:num_experts]
    starts = torch.cumsum(counts, 0) - counts
    starts = torch.cat([starts, starts.new_zeros(1)])
    rank = torch.empty(S, dtype=torch.long, device=dev)
    rank[order] = torch.arange(S, device=dev) - starts[skey]
    ec = e.clamp(min=0)
    if base is not None:
        rank = rank + base.long()[ec]
    slot = torch.where(valid, rank, torch.full_like(rank, -1))
    keep = valid & (slot >= 0) & (slot < capacity)
    tok = torch.arange(S, device=dev, dtype=torch.int32)
    src[(ec * capacity + slot)[keep]] = tok[keep]
    return slot.int(), counts.int(), src


def assign_slots(expert: Tensor, num_experts: int, capacity: int,
                 base: Optional[Tensor] = None,
                 src: Optional[Tensor] = None
                 ) -> Tuple[Tensor, Tensor, Tensor]:
    """Queue positions for one routing choice.

    expert  int32 (S,): chosen expert, -1 = token not routed
    base    int32 (E,) or None: queue position at which this call's
            tokens start (top-2 passes the first call's ``counts``)
    src     an earlier call's ``src`` to continue filling, or None for a
            fresh one

    Returns ``(slot, counts, src)``: ``slot`` int32 (S,) is the position
    in the expert's queue in token order plus ``base``, before any
    capacity test (-1 for unrouted tokens); ``counts`` int32 (E,) the
    tokens choosing each expert in this call, before dropping; ``src``
    int32 (E*capacity,) with ``src[expert*capacity + slot] = token`` for
    every token with ``0 <= slot < capacity`` and -1 elsewhere.
    """
    if expert.dim() != 1 or expert.dtype != torch.int32:
        raise ValueError("expert must be a 1-d int32 tensor")
    num_experts, capacity = int(num_experts), int(capacity)
    if num_experts < 1 or capacity < 1:
        raise ValueError("num_experts and capacity must be positive")
    if num_experts * capacity >= 2 ** 31:
        raise ValueError("num_experts * capacity must be below 2**31")
    if base is not None and (base.dtype != torch.int32
                             or base.shape != (num_experts,)):
        raise ValueError("base must be int32 of shape (num_experts,)")
    if src is None:
        src = torch.full((num_experts * capacity,), -1, dtype=torch.int32,
                         device=expert.device)
    elif src.dtype != torch.int32 or src.shape != (num_experts * capacity,):
        raise ValueError("src must be int32 of shape (E*capacity,)")

    if expert.is_cuda:
        lib = native.require()
        expert = expert.contiguous()
        slot = torch.empty_like(expert)
        counts = torch.empty(num_experts, dtype=torch.int32,
                             device=expert.device)
        lib.moe_assign_slots(expert, num_experts, capacity,
                             None if base is None else base.contiguous(),
                             slot, counts, src)
        return slot, counts, src
    return _assign_slots_torch(expert, num_experts, capacity, base, src)


# ---------------------------------------------------------------------------
# row movement
# ---------------------------------------------------------------------------

def _acc_dtype(rows: Tensor, w: Optional[Tensor] = None):
    """f32 accumulation for f16/bf16/f32 rows, f64 for f64 rows."""
    acc = torch.promote_types(rows.dtype, torch.float32)
    if w is not None:
        acc = torch.promote_types(acc, w.dtype)
    return acc


def _row_weights(w: Tensor, dest: Tensor, src: Tensor) -> Tensor:
    """Per-row weight: w[j, src[r]] for the j with dest[j, src[r]] == r."""
    s = src.long().clamp(min=0)
    wr = w[0][s]
    if w.shape[0] == 2:
        rows = torch.arange(src.numel(), device=src.device)
        wr = torch.where(dest[0].long()[s] == rows, wr, w[1][s])
    return wr


def gather_rows(x: Tensor, src: Tensor, w: Optional[Tensor] = None,
                dest: Optional[Tensor] = None) -> Tensor:
    """out[r] = src[r] >= 0 ? scale(r) * x[src[r]] : 0, where scale is 1
    without ``w`` and otherwise the weight of the choice that put token
    ``src[r]`` into row ``r``."""
    x = x.contiguous()
    if _native_rows(x):
        out = torch.empty((src.numel(), x.shape[1]), dtype=x.dtype,
                          device=x.device)
        native.lib().moe_gather_rows(
            x, src, out, None if w is None else w.float().contiguous(),
            None if dest is None else dest.contiguous())
        return out
    rows = x.index_select(0, src.long().clamp(min=0))
    if w is not None:
        acc = _acc_dtype(x, w)
        rows = (rows.to(acc)
                * _row_weights(w, dest, src).to(acc).unsqueeze(1)
                ).to(x.dtype)
    return torch.where((src >= 0).unsqueeze(1), rows,
                       torch.zeros_like(rows))


def combine_rows(eo: Tensor, dest: Tensor,
                 w: Optional[Tensor] = None) -> Tensor:
    """out[s] = sum_j (dest[j,s] >= 0 ? w[j,s] * eo[dest[j,s]] : 0);
    ``w`` absent means 1."""
    eo = eo.contiguous()
    k, S = dest.shape
    if _native_rows(eo):
        out = torch.empty((S, eo.shape[1]), dtype=eo.dtype,
                          device=eo.device)
        native.lib().moe_combine_rows(
            eo, dest.contiguous(), out,
            None if w is None else w.float().contiguous())
        return out
    acc = _acc_dtype(eo, w)
    out = None
    for j in range(k):
        term = eo.index_select(0, dest[j].long().clamp(min=0)).to(acc)
        if w is not None:
            term = term * w[j].to(acc).unsqueeze(1)
        term = torch.where((dest[j] >= 0).unsqueeze(1), term,
                           torch.zeros_like(term))
        out = term if out is None else out + term
    return out.to(eo.dtype)


def row_dot(g: Tensor, eo: Tensor, dest: Tensor) -> Tensor:
    """gw[j,s] = dest[j,s] >= 0 ? sum_m g[s,m] * eo[dest[j,s],m] : 0."""
    g = g.contiguous()
    eo = eo.contiguous()
    k, S = dest.shape
    if _native_rows(g, eo):
        gw = torch.empty((k, S), dtype=torch.float32, device=g.device)
        native.lib().moe_row_dot(g, eo, dest.contiguous(), gw)
        return gw
    acc = _acc_dtype(eo)
    ga = g.to(acc)
    gw = [(ga * eo.index_select(0, dest[j].long().clamp(min=0)).to(acc))
          .sum(1) for j in range(k)]
    gw = torch.stack(gw)
    return torch.where(dest >= 0, gw, torch.zeros_like(gw))


class _Dispatch(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, src, dest):
        ctx.dest = dest
        return gather_rows(x, src)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        return combine_rows(grad, ctx.dest), None, None


class _Combine(torch.autograd.Function):
    @staticmethod
    def forward(ctx, eo, weights, dest, src):
        ctx.save_for_backward(eo, weights)
        ctx.dest, ctx.src = dest, src
        return combine_rows(eo, dest, weights)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        eo, weights = ctx.saved_tensors
        g_eo = g_w = None
        if ctx.needs_input_grad[0]:
            g_eo = gather_rows(grad, ctx.src, weights, ctx.dest)
        if ctx.needs_input_grad[1]:
            g_w = row_dot(grad, eo, ctx.dest).to(weights.dtype)
        return g_eo, g_w, None, None


def _check_rows(rows: Tensor, n: int, what: str):
    if rows.dim() != 2 or rows.shape[0] != n:
        raise ValueError("%s must have shape (%d, M), got %s"
                         % (what, n, tuple(rows.shape)))


def dispatch(x: Tensor, plan: RoutingPlan) -> Tensor:
    """Move token rows ``(S, M)`` into their expert queues ``(E*C, M)``;
    empty slots are zero. Differentiable in ``x``."""
    _check_rows(x, plan.dest.shape[1], "x")
    return _Dispatch.apply(x, plan.src, plan.dest)


def combine(expert_out: Tensor, plan: RoutingPlan) -> Tensor:
    """Weighted sum of each token's ``k`` expert rows: ``(E*C, M) ->
    (S, M)``. Differentiable in ``expert_out`` and ``plan.weights``."""
    _check_rows(expert_out, plan.src.numel(), "expert_out")
    return _Combine.apply(expert_out, plan.weights, plan.dest, plan.src)
