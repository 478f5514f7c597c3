"""The activation behind a transformer MLP's first Linear as HIP kernels,
over rows ``[R, C]``::

    z = f32(h) + f32(bias)        a = gelu(z)
    dh = dy * gelu'(z)            dbias = sum over rows of dy * gelu'(z)

* :func:`forward`   one kernel: reads ``h``, writes ``a``;
* :func:`backward`  one kernel for ``dh``, which forms ``z`` again from ``h``
  and ``bias`` (nothing but ``h`` is kept), and a small second one for
  ``dbias``, which sums the f32 values before their rounding.

``h`` is the Linear's output without its bias and ``bias`` that bias, f32 or
in the dtype of ``h`` (f32 over a bf16 ``h`` is what autocast hands over), or
None for plain GELU. ``approximate`` is ``"none"`` (erf) or ``"tanh"``, as in
``torch.nn.functional.gelu`` and with its constants. Arithmetic is f32 with
one rounding per stored value; sums are deterministic. Any ``C`` that is a
multiple of 8 is taken.

:func:`kernels_apply` says whether the kernels of
``csrc/bias_gelu_kernels.hip`` take a call (mandatory on a GPU machine: a
missing extension raises, see ops/native.py); the caller keeps its torch
path for everything they decline.
"""

from typing import Optional, Tuple

import torch
from torch import Tensor

from . import native

_KERNEL_DTYPES = (torch.float32, torch.float16, torch.bfloat16)
_FORMS = ("none", "tanh")

# BAGUA_BG_BLOCK, BAGUA_BG_TILE_CHUNKS * 8, BAGUA_BG_MAX_GRID and
# BAGUA_BG_PARTIAL_BYTES of csrc/launchers.h, for callers that size a problem
# by them. A block has BLOCK threads; one takes 8 columns of a row, 64
# threads lie along a row (for C < 512 the next power of two at or above
# C / 8) and the others take further rows, so a block covers TILE_COLS
# columns of BLOCK // 64 rows or more. A grid has at most MAX_GRID blocks
# (column tiles times row blocks) and strides over the rows two at a time;
# with a bias gradient its row blocks are also held to PARTIAL_BYTES of f32
# partial sums, 4 * C bytes each.
BLOCK = 256
TILE_COLS = 512
MAX_GRID = 1024
PARTIAL_BYTES = 2 << 20


def kernels_apply(h: Tensor, bias: Optional[Tensor],
                  approximate: str = "none") -> bool:
    """True when the HIP kernels take ``gelu(h + bias, approximate)`` over
    the last dimension's rows. Raises on a GPU machine without the extension
    rather than falling back. Autocast does not matter: no
    autocast-sensitive op runs on this path."""
    if approximate not in _FORMS:
        return False
    if not h.is_cuda or h.dtype not in _KERNEL_DTYPES or h.dim() < 1:
        return False
    c = h.shape[-1]
    if c % 8 != 0 or c < 8 or not 0 < h.numel() < 2 ** 31:
        return False
    if not h.is_contiguous() or h.data_ptr() % 16 != 0:
        return False
    if bias is not None and not (
            bias.device == h.device and bias.dim() == 1
            and bias.shape[0] == c and bias.is_contiguous()
            and bias.dtype in (torch.float32, h.dtype)):
        return False
    native.require()
    return True


def forward(h: Tensor, bias: Optional[Tensor],
            approximate: str = "none") -> Tensor:
    """``a`` in the shape and dtype of ``h``."""
    a = torch.empty_like(h)
    c = h.shape[-1]
    native.lib().bias_gelu_forward(h.view(-1, c), bias,
                                   approximate == "tanh", a.view(-1, c))
    return a


def backward(dy: Tensor, h: Tensor, bias: Optional[Tensor],
             approximate: str = "none", want_bias: bool = True
             ) -> Tuple[Tensor, Optional[Tensor]]:
    """``(dh, dbias)``; ``dbias`` in the dtype of ``bias``, None without a
    bias or when not wanted. ``dy`` is contiguous and aligned as ``h`` is."""
    dh = torch.empty_like(h)
    dbias = (torch.empty_like(bias)
             if want_bias and bias is not None else None)
    c = h.shape[-1]
    native.lib().bias_gelu_backward(dy.view(-1, c), h.view(-1, c), bias,
                                    approximate == "tanh", dh.view(-1, c),
                                    dbias)
    return dh, dbias
