"""A transformer sub-layer's tail as HIP kernels, over rows ``[R, H]``::

    s = x + keep * (h + bias) / (1 - p)      # keep ~ Bernoulli(1 - p)
    y = (s - mean(s)) * rstd(s) * gamma + beta

* :func:`forward`   one kernel: reads ``x`` and ``h``, writes ``y``, ``s``
  (kept for backward), f32 ``mean``/``rstd`` per row and, with dropout, a
  keep mask of a byte per 8 elements;
* :func:`backward`  one kernel for ``dx`` and ``dh`` and a small second one
  for ``dgamma``, ``dbeta`` and ``dbias``; it reads the mask and never draws
  again.

``x`` is the residual stream, ``h`` a Linear's output without its bias and
``bias`` that bias. ``x``, ``s`` and ``y`` share one dtype; ``h`` has it too,
or is f16/bf16 under an f32 ``x`` (what autocast hands over). Each of
``bias``, ``gamma`` and ``beta`` may be None and is f32 or has the dtype of
the tensor it goes with. Without ``h`` this is plain LayerNorm. Arithmetic
is f32 with one rounding per stored value; sums are deterministic.

The dropout bits are Philox4x32-10 of the element's row-major index, keyed
by a 64-bit seed that the kernel reads from device memory: the mask depends
on (seed, index, p) alone. :func:`forward` draws the seed with a torch random
op on the device, so it follows ``torch.manual_seed`` and survives graph
capture.

:func:`kernels_apply` says whether the kernels of
``csrc/layernorm_kernels.hip`` take a call (mandatory on a GPU machine: a
missing extension raises, see ops/native.py); the caller keeps its torch
path for everything they decline.
"""

from typing import Optional, Tuple

import torch
from torch import Tensor

from . import native

_KERNEL_DTYPES = (torch.float32, torch.float16, torch.bfloat16)

# BAGUA_LN_HMAX, BAGUA_LN_WAVES and BAGUA_LN_FWD_MAX_GRID of
# csrc/launchers.h: the longest row, the rows a block works on at a time and
# the cap on the forward kernel's blocks, for callers that size a problem by
# them
HMAX = 4096
WAVES_PER_BLOCK = 4
FWD_MAX_GRID = 2048


def _column_vector_ok(t: Optional[Tensor], h: int, goes_with: Tensor) -> bool:
    return t is None or (
        t.device == goes_with.device and t.dim() == 1 and t.shape[0] == h
        and t.is_contiguous()
        and t.dtype in (torch.float32, goes_with.dtype))


def kernels_apply(x: Tensor, normalized_shape, branch: Optional[Tensor],
                  branch_bias: Optional[Tensor], weight: Optional[Tensor],
                  bias: Optional[Tensor], p: float) -> bool:
    """True when the HIP kernels take ``layer_norm(x + dropout(branch +
    branch_bias, p))`` over ``normalized_shape``. Raises on a GPU machine
    without the extension rather than falling back. Autocast does not
    matter: no autocast-sensitive op runs on this path."""
    if not x.is_cuda or x.dtype not in _KERNEL_DTYPES:
        return False
    if len(normalized_shape) != 1 or x.dim() < 1:
        return False
    h = normalized_shape[0]
    if x.shape[-1] != h or h % 8 != 0 or not 8 <= h <= HMAX:
        return False
    if not 0 < x.numel() < 2 ** 31:
        return False
    if not x.is_contiguous() or x.data_ptr() % 16 != 0:
        return False
    if not 0.0 <= p < 1.0:
        return False
    if branch is None:
        if branch_bias is not None:
            return False
    else:
        if (branch.shape != x.shape or branch.device != x.device
                or not branch.is_contiguous() or branch.data_ptr() % 16 != 0):
            return False
        if branch.dtype != x.dtype and not (
                x.dtype == torch.float32
                and branch.dtype in (torch.float16, torch.bfloat16)):
            return False
        if not _column_vector_ok(branch_bias, h, branch):
            return False
    if not (_column_vector_ok(weight, h, x)
            and _column_vector_ok(bias, h, x)):
        return False
    native.require()
    return True


def draw_seed(device) -> Tensor:
    """One int64 on ``device`` from torch's generator for it; no host read."""
    return torch.empty(1, dtype=torch.int64, device=device).random_()


def forward(x: Tensor, h: Optional[Tensor], bias: Optional[Tensor],
            gamma: Optional[Tensor], beta: Optional[Tensor], p: float,
            eps: float, seed: Optional[Tensor] = None
            ) -> Tuple[Tensor, Tensor, Tensor, Tensor, Optional[Tensor]]:
    """``(y, s, mean, rstd, mask)`` for ``x`` and ``h`` of shape ``[R, H]``.
    ``s`` is ``x`` itself without ``h``. ``mask`` is None for ``p == 0``,
    else uint8 ``[R, H / 8]``, bit ``k`` of byte ``j`` set where element
    ``8 j + k`` of the row is kept. ``seed`` (one int64 on the device) is
    drawn here when not given."""
    rows = x.shape[0]
    y = torch.empty_like(x)
    s = x if h is None else torch.empty_like(x)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty_like(mean)
    mask = None
    if h is None or p == 0.0:
        p, seed = 0.0, None
    else:
        if seed is None:
            seed = draw_seed(x.device)
        mask = torch.empty(rows, x.shape[1] // 8, dtype=torch.uint8,
                           device=x.device)
    native.lib().ln_forward(x, h, bias, gamma, beta, seed, p, eps, y,
                            None if h is None else s, mean, rstd, mask)
    return y, s, mean, rstd, mask


def backward(grad_output: Tensor, s: Tensor, mean: Tensor, rstd: Tensor,
             gamma: Optional[Tensor], mask: Optional[Tensor], p: float,
             branch_dtype: Optional[torch.dtype] = None,
             want_gamma: bool = False, beta: Optional[Tensor] = None,
             bias: Optional[Tensor] = None
             ) -> Tuple[Tensor, Optional[Tensor], Optional[Tensor],
                        Optional[Tensor], Optional[Tensor]]:
    """``(dx, dh, dgamma, dbeta, dbias)``. ``branch_dtype`` is the dtype of
    the forward's ``h`` (None without one, and then ``dh`` is None);
    without dropout and with one dtype, ``dh`` is ``dx``, one tensor.
    ``dgamma`` is formed when ``want_gamma``, ``dbeta`` and ``dbias`` when
    ``beta`` and ``bias`` (the parameters, for their dtypes) are given."""
    has_branch = branch_dtype is not None
    dx = torch.empty_like(s)
    dh = None
    if has_branch and (mask is not None or branch_dtype != s.dtype):
        dh = torch.empty_like(s, dtype=branch_dtype)
    dgamma = (torch.empty_like(gamma)
              if want_gamma and gamma is not None else None)
    dbeta = None if beta is None else torch.empty_like(beta)
    dbias = None if bias is None or not has_branch else torch.empty_like(bias)
    native.lib().ln_backward(grad_output, s, mean, rstd, gamma, mask,
                             p if mask is not None else 0.0, has_branch, dx,
                             dh, dgamma, dbeta, dbias)
    return dx, (dx if has_branch and dh is None else dh), dgamma, dbeta, dbias
