"""GELU that takes the bias of the Linear in front of it into its own
kernels: ``forward(h, bias)`` is

    gelu(h + bias, approximate=self.approximate)

the middle of a transformer MLP, with ``h`` the output of the first Linear
computed without its bias. On the GPU, where ``ops.bias_gelu.kernels_apply``
takes the call, that is one ``autograd.Function`` over the HIP kernels of
``ops/bias_gelu.py``: one pass forward, and one backward that also leaves the
bias gradient's column sums, so that no separate pass over the gradient forms
them. ``h + bias`` is formed in f32 and never stored; backward keeps ``h``
alone. Everywhere else (the CPU, shapes the kernels decline) it is that
torch chain. Without a bias it is plain GELU.

No parameters: a ``state_dict`` has no key for it, as for ``nn.GELU``.
"""

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..ops import bias_gelu as bg_ops

__all__ = ["FusedBiasGELU"]


class FusedBiasGELU(nn.GELU):
    def forward(self, h, bias=None, kernels=True):
        """``kernels=False`` runs the torch chain whatever the input, which
        without a bias is ``nn.GELU.forward`` itself."""
        if kernels and bg_ops.kernels_apply(h, bias, self.approximate):
            return _BiasGELUFn.apply(h, bias, self.approximate)
        if bias is None:
            return super().forward(h)
        return F.gelu(h + bias, approximate=self.approximate)


class _BiasGELUFn(torch.autograd.Function):
    """On the kernel path only: the caller has asked
    ``bg_ops.kernels_apply``."""

    @staticmethod
    def forward(ctx, h, bias, approximate):
        ctx.save_for_backward(h, bias)
        ctx.approximate = approximate
        return bg_ops.forward(h, bias, approximate)

    @staticmethod
    def backward(ctx, grad_output):
        h, bias = ctx.saved_tensors
        with torch.no_grad():
            grad_output = grad_output.contiguous()
            if grad_output.data_ptr() % 16 != 0:
                grad_output = grad_output.clone()
            dh, dbias = bg_ops.backward(grad_output, h, bias, ctx.approximate,
                                        ctx.needs_input_grad[1])
        return dh if ctx.needs_input_grad[0] else None, dbias, None
