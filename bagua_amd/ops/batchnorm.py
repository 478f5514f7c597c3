"""Batch normalisation over a batch that is spread across ranks, as four
HIP kernel roles around the two SUM-allreduces of
``contrib/sync_batchnorm.py``:

* :func:`stats`            per-channel ``(sum x, sum x*x, count)`` of the
  local batch, the vector that is allreduced;
* :func:`apply`            ``y = (x - mean) * invstd * w + b`` from the
  reduced vector; also keeps ``mean``/``invstd`` for backward and moves the
  running statistics;
* :func:`backward_reduce`  ``(sum dy, sum dy * (x - mean))``, the second
  allreduced vector, and the parameter gradients from the local sums;
* :func:`backward_apply`   ``dx`` from the reduced sums.

Forward reads ``x`` twice and writes ``y``; backward reads ``dy`` and ``x``
twice and writes ``dx``, all in the input's dtype, with f32 arithmetic and
deterministic sums. The kernels of ``csrc/batchnorm_kernels.hip`` see the
input as rows of channels (4-d channels-last, or inner size 1) or as
NCHW-contiguous planes; outputs keep the input's memory format.

:func:`apply_act`, :func:`backward_reduce_act` and :func:`backward_apply_act`
are the same three roles with ``relu(bn(x))`` or ``relu(bn(x) + z)`` fused
in: the add and the ReLU happen in f32 before the one rounding, backward
reads the sign of ``y`` (a byte per 16 bytes of it in the rows layout, ``y``
itself in the planes layout) and writes the residual's gradient in the pass
that writes ``dx``. :func:`stats` serves both.

:func:`kernels_apply` says whether they take a call (mandatory on a GPU
machine: a missing extension raises, see ops/native.py); the caller keeps
its torch path for everything they decline.
"""

from typing import Optional, Tuple

import torch
from torch import Tensor

from . import native

_KERNEL_DTYPES = (torch.float32, torch.float16, torch.bfloat16)

# cap on the row-blocks of the rows layout's apply kernels, BN_APPLY_MAX_GRID
# of csrc/batchnorm_kernels.hip, for callers that size a problem by it
ROWS_APPLY_MAX_GRID = 2048


def _vec(dtype) -> int:
    return 128 // torch.finfo(dtype).bits  # elements per 16 bytes


def layout_of(input: Tensor) -> Optional[str]:
    """``"rows"``, ``"planes"`` or None for a layout the kernels decline."""
    if input.dim() < 2 or input.numel() == 0:
        return None
    inner = input.numel() // (input.shape[0] * input.shape[1])
    channels_last = (input.dim() == 4 and not input.is_contiguous()
                     and input.is_contiguous(
                         memory_format=torch.channels_last))
    if channels_last or (inner == 1 and input.is_contiguous()):
        if input.shape[1] % _vec(input.dtype) != 0 \
                or input.data_ptr() % 16 != 0:
            return None
        return "rows"
    return "planes" if input.is_contiguous() else None


def _channel_vector_ok(t: Optional[Tensor], input: Tensor) -> bool:
    return t is None or (
        t.device == input.device and t.dim() == 1
        and t.shape[0] == input.shape[1] and t.is_contiguous()
        and t.dtype in (torch.float32, input.dtype))


def kernels_apply(input: Tensor, weight: Optional[Tensor],
                  bias: Optional[Tensor], running_mean: Optional[Tensor],
                  running_var: Optional[Tensor],
                  momentum: Optional[float]) -> bool:
    """True when the HIP kernels take this call. Raises on a GPU machine
    without the extension rather than falling back. Autocast does not
    matter: no autocast-sensitive op runs on this path, and bf16 input with
    f32 parameters is what autocast hands over."""
    if not input.is_cuda or input.dtype not in _KERNEL_DTYPES:
        return False
    if momentum is None or input.numel() >= 2 ** 31:
        return False
    if layout_of(input) is None:
        return False
    if not all(_channel_vector_ok(t, input)
               for t in (weight, bias, running_mean, running_var)):
        return False
    if (running_mean is None) != (running_var is None):
        return False
    if running_mean is not None and running_mean.dtype != running_var.dtype:
        return False
    native.require()
    return True


def _f32(input: Tensor, numel: int) -> Tensor:
    return torch.empty(numel, dtype=torch.float32, device=input.device)


def like_input(t: Tensor, input: Tensor) -> Tensor:
    """``t`` in ``input``'s memory format and, in the rows layout, aligned
    as the kernels need it; ``t`` itself when it already is."""
    rows = layout_of(input) == "rows"
    if rows and input.dim() == 4 and not input.is_contiguous():
        t = t.contiguous(memory_format=torch.channels_last)
    else:
        t = t.contiguous()
    if rows and t.data_ptr() % 16 != 0:
        t = t.clone(memory_format=torch.preserve_format)
    return t


def stats(input: Tensor) -> Tensor:
    """f32 ``[2C + 1]``: per-channel sum, sum of squares, and the number of
    elements per channel of this (local) batch."""
    out = _f32(input, 2 * input.shape[1] + 1)
    native.lib().bn_stats(input, out)
    return out


def apply(input: Tensor, stats: Tensor, weight: Optional[Tensor],
          bias: Optional[Tensor], running_mean: Optional[Tensor],
          running_var: Optional[Tensor], momentum: float,
          eps: float) -> Tuple[Tensor, Tensor]:
    """``(y, mean_invstd)`` from the reduced ``stats``; ``mean_invstd`` is
    f32 ``[2C]``. The running statistics are updated in place."""
    y = torch.empty_like(input)
    mean_invstd = _f32(input, 2 * input.shape[1])
    native.lib().bn_apply(input, y, stats, mean_invstd, weight, bias,
                          running_mean, running_var, momentum, eps)
    return y, mean_invstd


def backward_reduce(grad_output: Tensor, input: Tensor, mean_invstd: Tensor,
                    weight: Optional[Tensor] = None,
                    bias: Optional[Tensor] = None
                    ) -> Tuple[Tensor, Optional[Tensor], Optional[Tensor]]:
    """``(packed, grad_weight, grad_bias)``: f32 ``[2C]`` sums of ``dy`` and
    ``dy * (x - mean)`` of the local batch, and the gradients of the given
    parameters, in their dtypes, from the same local sums."""
    packed = _f32(input, 2 * input.shape[1])
    gw = None if weight is None else torch.empty_like(weight)
    gb = None if bias is None else torch.empty_like(bias)
    native.lib().bn_backward_reduce(grad_output, input, mean_invstd, packed,
                                    gw, gb)
    return packed, gw, gb


def backward_apply(grad_output: Tensor, input: Tensor, packed: Tensor,
                   stats: Tensor, mean_invstd: Tensor,
                   weight: Optional[Tensor]) -> Tensor:
    """``dx`` from the reduced ``packed`` sums and the count in ``stats``."""
    dx = torch.empty_like(input)
    native.lib().bn_backward_apply(grad_output, input, dx, packed, stats,
                                   mean_invstd, weight)
    return dx


def apply_act(input: Tensor, stats: Tensor, weight: Optional[Tensor],
              bias: Optional[Tensor], running_mean: Optional[Tensor],
              running_var: Optional[Tensor], momentum: float, eps: float,
              residual: Optional[Tensor] = None
              ) -> Tuple[Tensor, Tensor, Tensor]:
    """:func:`apply` with the activation fused: ``(y, mean_invstd, act)``
    with ``y = relu(bn(input) [+ residual])``, the add in f32 before the one
    rounding. ``residual`` is in ``input``'s memory format
    (:func:`like_input`). ``act`` is what backward needs of ``y``, its sign:
    in the rows layout a ``uint8`` mask ``[rows, C / V]``, one byte per
    16-byte vector with bit ``k`` set where element ``k`` of the stored
    ``y`` is above zero; in the planes layout ``y`` itself."""
    y = torch.empty_like(input)
    mean_invstd = _f32(input, 2 * input.shape[1])
    mask = None
    if layout_of(input) == "rows":
        c = input.shape[1]
        mask = torch.empty(input.numel() // c, c // _vec(input.dtype),
                           dtype=torch.uint8, device=input.device)
    native.lib().bn_apply_act(input, y, stats, mean_invstd, weight, bias,
                              running_mean, running_var, momentum, eps,
                              residual, mask)
    return y, mean_invstd, y if mask is None else mask


def backward_reduce_act(grad_output: Tensor, input: Tensor, act: Tensor,
                        mean_invstd: Tensor,
                        weight: Optional[Tensor] = None,
                        bias: Optional[Tensor] = None
                        ) -> Tuple[Tensor, Optional[Tensor],
                                   Optional[Tensor]]:
    """:func:`backward_reduce` of ``d = grad_output`` where ``y > 0`` and 0
    elsewhere, read from :func:`apply_act`'s ``act``."""
    packed = _f32(input, 2 * input.shape[1])
    gw = None if weight is None else torch.empty_like(weight)
    gb = None if bias is None else torch.empty_like(bias)
    native.lib().bn_backward_reduce_act(grad_output, input, act, mean_invstd,
                                        packed, gw, gb)
    return packed, gw, gb


def backward_apply_act(grad_output: Tensor, input: Tensor, act: Tensor,
                       packed: Tensor, stats: Tensor, mean_invstd: Tensor,
                       weight: Optional[Tensor], want_residual_grad: bool
                       ) -> Tuple[Tensor, Optional[Tensor]]:
    """``(dx, dz)``: :func:`backward_apply` of the same ``d``, and, where
    wanted, ``d`` itself as the residual's gradient, from the same pass."""
    dx = torch.empty_like(input)
    dz = torch.empty_like(input) if want_residual_grad else None
    native.lib().bn_backward_apply_act(grad_output, input, act, dx, packed,
                                       stats, mean_invstd, weight, dz)
    return dx, dz
