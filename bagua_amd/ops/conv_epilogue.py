"""Fused epilogue of a ``Conv2d -> ReLU [-> MaxPool2d(2, 2)]`` stage.

torch runs the stage as separate memory-bound passes over the conv output:
bias ``add_``, ``relu_``, ``max_pool2d`` (which also writes int64 indices)
and, backward, ``max_pool2d`` backward, ``threshold_backward`` and the bias
gradient's ``sum((0, 2, 3))``. :func:`conv_bias_relu` does each direction
in one pass:

* forward   ``y = relu(conv_out + bias)`` in place on ``conv_out`` and,
  with ``pool``, ``p = max_pool2d(y, 2, 2)`` from the same pass, without
  indices;
* backward  ``dx = (y <= 0) ? 0 : g``; with ``pool`` the window's winner is
  found again from the saved ``y``; the bias gradient ``sum(dx)`` is
  accumulated on the way.

``y``, ``p`` and ``dx`` are bit for bit those of the torch chain. The bias
gradient is a deterministic f32 sum rounded once; its order differs from
torch's reduction, so it can differ from it in the last bit
(``torch_bias_grad=True`` leaves it to ``dx.sum((0, 2, 3))``).

Two paths, like the rest of ``bagua_amd.ops``: the gfx950 kernels of
``csrc/epilogue_kernels.hip`` when :func:`kernels_apply` holds (mandatory
on a GPU machine: a missing extension raises, see ops/native.py), and an
equivalent torch implementation for CPU, other dtypes and everything the
kernels decline.
"""

import torch
import torch.nn.functional as F
from torch import Tensor
from torch.autograd.function import once_differentiable

from . import native

_KERNEL_DTYPES = (torch.float32, torch.float16, torch.bfloat16)
# lanes of a block along C; more channel vectors than this are declined
_MAX_CHANNEL_VECTORS = 256


def _shape_ok(dtype, channels: int, height: int, width: int,
              pool: bool) -> bool:
    vec = 128 // torch.finfo(dtype).bits  # elements per 16 bytes
    if channels % vec != 0 or channels // vec > _MAX_CHANNEL_VECTORS:
        return False
    if pool and (height % 2 != 0 or width % 2 != 0):
        return False
    return True


def kernels_apply(conv_out: Tensor, bias: Tensor, pool: bool) -> bool:
    """True when the HIP kernels take this call. Raises on a GPU machine
    without the extension rather than falling back."""
    if not (conv_out.is_cuda and bias.is_cuda):
        return False
    if conv_out.dtype not in _KERNEL_DTYPES or bias.dtype != conv_out.dtype:
        return False
    if conv_out.dim() != 4 or bias.dim() != 1:
        return False
    if torch.is_autocast_enabled():
        return False
    n, c, h, w = conv_out.shape
    if bias.shape[0] != c or not bias.is_contiguous():
        return False
    if not _shape_ok(conv_out.dtype, c, h, w, pool):
        return False
    if conv_out.numel() == 0 or n * h * w >= 2 ** 31:
        return False
    if not conv_out.is_contiguous(memory_format=torch.channels_last):
        return False
    if conv_out.data_ptr() % 16 != 0:
        return False
    native.require()
    return True


def conv_eligible(x: Tensor, conv: torch.nn.Conv2d, pool: bool) -> bool:
    """Will :func:`kernels_apply` hold for the output of ``conv(x)``?
    Answered from the input, before the convolution runs, so that a model
    can keep its stock path for everything else."""
    if not x.is_cuda or x.dim() != 4 or conv.bias is None:
        return False
    w, b = conv.weight, conv.bias
    if x.dtype not in _KERNEL_DTYPES or w.dtype != x.dtype \
            or b.dtype != x.dtype:
        return False
    if torch.is_autocast_enabled():
        return False
    if conv.padding_mode != "zeros" or isinstance(conv.padding, str):
        return False
    if not x.is_contiguous(memory_format=torch.channels_last):
        return False
    out = []
    for i in range(2):
        span = conv.dilation[i] * (conv.kernel_size[i] - 1) + 1
        out.append((x.shape[2 + i] + 2 * conv.padding[i] - span)
                   // conv.stride[i] + 1)
    if out[0] < 1 or out[1] < 1 or x.shape[0] < 1:
        return False
    if not _shape_ok(x.dtype, conv.out_channels, out[0], out[1], pool):
        return False
    native.require()
    return True


def _channels_last(t: Tensor) -> Tensor:
    t = t.contiguous(memory_format=torch.channels_last)
    if t.data_ptr() % 16 != 0:
        t = t.clone(memory_format=torch.channels_last)
    return t


class _ConvBiasRelu(torch.autograd.Function):
    """apply(conv_out, bias, pool, torch_bias_grad) -> y | (y, p)

    ``conv_out`` is overwritten with ``y`` (marked dirty: the convolution's
    backward does not need its own output, the liberty an in-place ReLU
    takes too) and saved. autograd wants a dirtied input among the outputs,
    so with ``pool`` both ``y`` and ``p`` are returned."""

    @staticmethod
    def forward(ctx, conv_out, bias, pool, torch_bias_grad):
        ctx.set_materialize_grads(False)
        ctx.pool = pool
        ctx.torch_bias_grad = torch_bias_grad
        ctx.native = kernels_apply(conv_out, bias, pool)
        ctx.mark_dirty(conv_out)
        p = idx = None
        if ctx.native:
            lib = native.lib()
            if pool:
                n, c, h, w = conv_out.shape
                p = torch.empty((n, c, h // 2, w // 2), dtype=conv_out.dtype,
                                device=conv_out.device,
                                memory_format=torch.channels_last)
                lib.conv_bias_relu_pool_(conv_out, bias.detach(), p)
            else:
                lib.conv_bias_relu_(conv_out, bias.detach())
        else:
            conv_out.add_(bias.detach().view(1, -1, 1, 1))
            torch.relu_(conv_out)
            if pool:
                p, idx = F.max_pool2d(conv_out, 2, 2, return_indices=True)
        if pool:
            ctx.save_for_backward(conv_out, idx)
            return conv_out, p
        ctx.save_for_backward(conv_out)
        return conv_out

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        g = grads[-1]  # of p with pool, of y without
        if ctx.pool and grads[0] is not None:
            raise RuntimeError("conv_bias_relu: with pool only the pooled "
                               "output is differentiable")
        if g is None:
            return None, None, None, None
        y = ctx.saved_tensors[0]
        want_db = ctx.needs_input_grad[1]
        db = None
        if ctx.native:
            lib = native.lib()
            g = _channels_last(g)
            dx = torch.empty_like(y)
            if want_db and not ctx.torch_bias_grad:
                db = torch.empty(y.shape[1], dtype=y.dtype, device=y.device)
            (lib.conv_pool_relu_bwd if ctx.pool else lib.conv_relu_bwd)(
                g, y, dx, db)
        else:
            if ctx.pool:
                g = torch.ops.aten.max_pool2d_with_indices_backward(
                    g, y, [2, 2], [2, 2], [0, 0], [1, 1], False,
                    ctx.saved_tensors[1])
            dx = torch.ops.aten.threshold_backward(g, y, 0)
        if want_db and db is None:
            db = dx.sum((0, 2, 3))
        return dx, db, None, None


def conv_bias_relu(conv_out: Tensor, bias: Tensor, pool: bool = False,
                   torch_bias_grad: bool = False) -> Tensor:
    """``relu(conv_out + bias)``, max-pooled 2x2/stride 2 with ``pool``.

    ``conv_out`` (N, C, H, W) is the bias-free convolution result and is
    overwritten; it must not be a leaf that requires grad. Differentiable
    in ``conv_out`` and ``bias``. ``torch_bias_grad`` makes the kernel path
    take the bias gradient from ``dx.sum((0, 2, 3))``, which is bitwise what
    the unfused chain computes."""
    out = _ConvBiasRelu.apply(conv_out, bias, bool(pool),
                              bool(torch_bias_grad))
    return out[1] if pool else out
