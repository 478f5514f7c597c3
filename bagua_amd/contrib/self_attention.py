"""Self-attention that takes the ``qkv`` Linear's output as it lies and a
length per sequence: ``forward(qkv, seq_lens)`` with ``qkv`` ``(B, S, 3 * H)``
laid out ``(3, num_heads, head_dim)`` is, for each sequence of length ``L``
and each head,

    softmax(q K[:L]^T / sqrt(head_dim)) V[:L]      in rows below L, zeros behind

as ``(B, S, H)``. Padded keys are not attended, ``dout`` at padded rows is
ignored, the gradient there is zero, and nothing stored in padded rows of
``qkv`` reaches a result. ``seq_lens`` is ``(B,)`` integers on the device of
``qkv`` (never read on the host), or None for full sequences.

On the GPU, where ``ops.attention.kernels_apply`` takes the call (f16 and
bf16, ``head_dim`` 64), that is one ``autograd.Function`` over the MFMA
kernels of ``ops/attention.py``: they read ``qkv`` in place, write the output
at its heads' columns and the gradient as one packed ``dqkv``, so no
transpose, copy or ``cat`` surrounds them, and they skip padded keys and
padded query tiles. Everywhere else it is ``ops.attention.reference``, SDPA
with a key mask.

No parameters: a ``state_dict`` has no key for it.
"""

import torch
import torch.nn as nn

from ..ops import attention as att_ops

__all__ = ["PackedSelfAttention"]


class PackedSelfAttention(nn.Module):
    def __init__(self, num_heads: int):
        super().__init__()
        self.num_heads = num_heads

    def forward(self, qkv, seq_lens=None, kernels=True):
        """``kernels=False`` runs the torch form whatever the input."""
        if kernels and att_ops.kernels_apply(qkv, self.num_heads, seq_lens):
            return _PackedAttentionFn.apply(qkv, seq_lens, self.num_heads)
        return att_ops.reference(qkv, self.num_heads, seq_lens)

    def extra_repr(self):
        return "num_heads=%d" % self.num_heads


class _PackedAttentionFn(torch.autograd.Function):
    """On the kernel path only: the caller has asked
    ``att_ops.kernels_apply``."""

    @staticmethod
    def forward(ctx, qkv, seq_lens, num_heads):
        out, lse = att_ops.forward(qkv, num_heads, seq_lens)
        ctx.save_for_backward(qkv, out, lse, seq_lens)
        ctx.num_heads = num_heads
        return out

    @staticmethod
    def backward(ctx, grad_output):
        qkv, out, lse, seq_lens = ctx.saved_tensors
        with torch.no_grad():
            grad_output = grad_output.contiguous()
            if grad_output.data_ptr() % 16 != 0:
                grad_output = grad_output.clone()
            dqkv = att_ops.backward(grad_output, qkv, out, lse, seq_lens,
                                    ctx.num_heads)
        return dqkv, None, None
