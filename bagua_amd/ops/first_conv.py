"""The first stage of a VGG-style network, ``Conv2d(3, 64, 3, padding=1) ->
ReLU`` on the image, as one HIP kernel each way.

Set against the hardware this stage is the worst of the network: the
convolution is a few GFLOP, but its 64-channel output is the largest
activation there is, and the unfused chain passes over it five times
(convolution write, bias + ReLU in place, ``dx`` write, ``dx`` read by the
weight gradient). The image needs no gradient, so ``dx`` is needed by nothing
but this layer's own weight and bias gradients:

* forward   ``y = relu(bf16(bf16(conv(x, w)) + b))``, written once. The two
  roundings are those of the unfused chain; ``y`` differs from it only where
  the order of the f32 summation flips a rounding;
* backward  ``dx = (y <= 0) ? 0 : g`` is formed in registers from one read of
  ``g`` and ``y`` and goes straight into the weight- and bias-gradient sums
  (deterministic f32, rounded once to bf16). It is never written.

There is no torch implementation of this op: :func:`eligible` says whether
the gfx950 kernels of ``csrc/first_conv_kernels.hip`` take a call, and a
model keeps its existing path for everything else. On a GPU machine without
the extension it raises rather than declining (see ops/native.py).
"""

import torch
from torch import Tensor
from torch.autograd.function import once_differentiable

from . import native

IN_CHANNELS = 3
OUT_CHANNELS = 64


def _dense_weight(w: Tensor) -> bool:
    return w.is_contiguous() \
        or w.is_contiguous(memory_format=torch.channels_last)


def eligible(x: Tensor, conv: torch.nn.Conv2d) -> bool:
    """True when ``relu(conv(x))`` can run as :func:`first_conv_bias_relu`.
    Reads only metadata. Raises on a GPU machine without the extension."""
    if not x.is_cuda or x.dim() != 4 or x.requires_grad:
        return False
    if torch.is_autocast_enabled():
        return False
    w, b = conv.weight, conv.bias
    if b is None:
        return False
    if not (x.dtype == w.dtype == b.dtype == torch.bfloat16):
        return False
    if (conv.in_channels != IN_CHANNELS or conv.out_channels != OUT_CHANNELS
            or x.shape[1] != IN_CHANNELS
            or tuple(conv.kernel_size) != (3, 3)
            or tuple(conv.stride) != (1, 1)
            or isinstance(conv.padding, str)
            or tuple(conv.padding) != (1, 1)
            or tuple(conv.dilation) != (1, 1) or conv.groups != 1
            or conv.padding_mode != "zeros"):
        return False
    n, _, h, wd = x.shape
    if n < 1 or h < 1 or wd < 1 or n * h * wd >= 2 ** 31:
        return False
    if not x.is_contiguous(memory_format=torch.channels_last):
        return False
    if x.data_ptr() % 16 != 0:
        return False
    if not _dense_weight(w) or not b.is_contiguous():
        return False
    native.require()
    return True


def _channels_last(t: Tensor) -> Tensor:
    t = t.contiguous(memory_format=torch.channels_last)
    if t.data_ptr() % 16 != 0:
        t = t.clone(memory_format=torch.channels_last)
    return t


class _FirstConvBiasRelu(torch.autograd.Function):
    """apply(x, weight, bias) -> y. Saves ``x`` and ``y``; ``x`` gets no
    gradient. The weight gradient comes back in ``weight``'s own strides, so
    that nothing downstream has to copy it."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.set_materialize_grads(False)
        y = native.require().first_conv_bias_relu(x, weight.detach(),
                                                  bias.detach())
        ctx.save_for_backward(x, y, weight)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        if g is None or not (ctx.needs_input_grad[1]
                             or ctx.needs_input_grad[2]):
            return None, None, None
        x, y, weight = ctx.saved_tensors
        dw, db = native.require().first_conv_bias_relu_bwd(
            _channels_last(g), y, x, weight)
        return (None, dw if ctx.needs_input_grad[1] else None,
                db if ctx.needs_input_grad[2] else None)


def first_conv_bias_relu(x: Tensor, weight: Tensor, bias: Tensor) -> Tensor:
    """``relu(conv2d(x, weight, padding=1) + bias)`` for a channels-last bf16
    image ``x`` (N, 3, H, W) and a (64, 3, 3, 3) weight. Differentiable in
    ``weight`` and ``bias`` only. The caller has asked :func:`eligible`."""
    return _FirstConvBiasRelu.apply(x, weight, bias)
