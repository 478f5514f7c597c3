"""LayerNorm that takes the dropout and the residual add in front of it into
its own kernels: ``forward(x, branch, branch_bias, p)`` is

    layer_norm(x + dropout(branch + branch_bias, p, self.training))

the tail of a transformer sub-layer, with ``branch`` the output of the
sub-layer's last Linear computed without its bias. On the GPU, where
``ops.layernorm.kernels_apply`` takes the call, that is one
``autograd.Function`` over the HIP kernels of ``ops/layernorm.py``: one pass
forward, one backward plus the column sums, all in f32 arithmetic with the
branch in its own dtype (bf16 under an f32 residual stream is what autocast
hands over, and nothing here depends on autocast's casting rules). Everywhere
else (the CPU, shapes the kernels decline, normalisation over more than one
dimension) it is that torch chain, which draws from torch's generator
exactly as ``nn.Dropout`` does. Without a branch it is plain LayerNorm.

Parameters and ``state_dict`` keys are those of ``nn.LayerNorm``.
"""

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..ops import layernorm as ln_ops

__all__ = ["FusedDropoutAddLayerNorm"]


class FusedDropoutAddLayerNorm(nn.LayerNorm):
    def forward(self, x, branch=None, branch_bias=None, p=0.0, kernels=True):
        """``kernels=False`` runs the torch chain whatever the input, which
        without a branch is ``nn.LayerNorm.forward`` itself."""
        if branch is None and branch_bias is not None:
            raise ValueError("branch_bias is the bias of a branch: pass the "
                             "branch with it")
        drop = p if self.training and branch is not None else 0.0
        if kernels and ln_ops.kernels_apply(
                x, self.normalized_shape, branch, branch_bias, self.weight,
                self.bias, drop):
            return _DropoutAddLayerNormFn.apply(
                x, branch, branch_bias, self.weight, self.bias, drop,
                self.eps)
        if branch is not None:
            if branch_bias is not None:
                branch = branch + branch_bias
            x = x + F.dropout(branch, p, self.training)
        return F.layer_norm(x, self.normalized_shape, self.weight, self.bias,
                            self.eps)


class _DropoutAddLayerNormFn(torch.autograd.Function):
    """On the kernel path only: the caller has asked
    ``ln_ops.kernels_apply``."""

    @staticmethod
    def forward(ctx, x, branch, branch_bias, weight, bias, p, eps):
        hidden = x.shape[-1]
        y, s, mean, rstd, mask = ln_ops.forward(
            x.view(-1, hidden),
            None if branch is None else branch.view(-1, hidden),
            branch_bias, weight, bias, p, eps)
        ctx.save_for_backward(s, mean, rstd, weight, bias, branch_bias, mask)
        ctx.p = p
        ctx.shape = x.shape
        ctx.branch_dtype = None if branch is None else branch.dtype
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, grad_output):
        s, mean, rstd, weight, bias, branch_bias, mask = ctx.saved_tensors
        need = ctx.needs_input_grad
        with torch.no_grad():
            grad_output = grad_output.reshape(s.shape).contiguous()
            if grad_output.data_ptr() % 16 != 0:
                grad_output = grad_output.clone()
            dx, dh, dweight, dbias, dbranch_bias = ln_ops.backward(
                grad_output, s, mean, rstd, weight, mask, ctx.p,
                ctx.branch_dtype, need[3], bias if need[4] else None,
                branch_bias if need[2] else None)
        # without dropout and with one dtype the branch's gradient is the
        # residual's: the same tensor object, so autograd sees it as shared
        grad_x = dx.view(ctx.shape)
        grad_branch = grad_x if dh is dx else (
            None if dh is None else dh.view(ctx.shape))
        return (grad_x if need[0] else None,
                grad_branch if need[1] else None,
                dbranch_bias, dweight, dbias, None, None)
