"""Self-attention over a packed ``qkv`` with a length per sequence, as HIP
kernels (``csrc/attention_kernels.hip``) and as torch.

``qkv`` is ``(B, S, 3 * H)`` with its last dimension laid out
``(3, num_heads, head_dim)``, as one Linear emits it. ``seq_lens`` is None
(every length is ``S``) or ``(B,)`` integers on ``qkv``'s device, each
clamped to ``[0, S]`` where it is used: nothing here reads a length on the
host. For sequence ``b`` of length ``L``, head by head::

    out[b, i] = softmax(q_i . K[:L]^T / sqrt(head_dim)) V[:L]     i < L
    out[b, i] = 0                                                 i >= L

``dout`` at rows ``>= L`` is ignored and ``dqkv`` there is zero. Nothing
stored at rows ``>= L`` of ``qkv`` reaches any result, NaN included.

* :func:`forward`   one kernel: ``out (B, S, H)`` written at each head's
  columns, and the f32 log-sum-exp ``(B, num_heads, S)`` of the scaled scores.
* :func:`backward`  three kernels (``delta``, ``dK`` and ``dV``, ``dQ``),
  which form the probabilities again from the log-sum-exp and write the three
  thirds of a packed ``dqkv (B, S, 3 * H)`` in place, zeros included.
* :func:`reference` the same semantics in torch ops, for everything the
  kernels decline.

:func:`kernels_apply` says whether the kernels take a call (mandatory on a
GPU machine: a missing extension raises, see ops/native.py).
"""

from typing import Optional, Tuple

import torch
import torch.nn.functional as F
from torch import Tensor

from . import native

_KERNEL_DTYPES = (torch.float16, torch.bfloat16)

# BAGUA_ATT_BLOCK_M, BAGUA_ATT_BLOCK_N and BAGUA_ATT_HEAD_DIM of
# csrc/launchers.h. A forward block has BLOCK_M queries (32 a wave) and goes
# through the keys BLOCK_N at a time; backward uses the same two numbers, its
# key blocks BLOCK_M keys over BLOCK_N queries at a time.
BLOCK_M = 128
BLOCK_N = 64
HEAD_DIM = 64


def _lens_ok(qkv: Tensor, seq_lens: Optional[Tensor]) -> bool:
    return seq_lens is None or (
        seq_lens.device == qkv.device and seq_lens.dim() == 1
        and seq_lens.shape[0] == qkv.shape[0]
        and not seq_lens.dtype.is_floating_point
        and not seq_lens.dtype.is_complex and seq_lens.dtype != torch.bool)


def kernels_apply(qkv: Tensor, num_heads: int,
                  seq_lens: Optional[Tensor] = None) -> bool:
    """True when the HIP kernels take this attention. Raises on a GPU machine
    without the extension rather than falling back."""
    if not qkv.is_cuda or qkv.dtype not in _KERNEL_DTYPES or qkv.dim() != 3:
        return False
    b, s, h3 = qkv.shape
    if not 1 <= num_heads <= 65535 or h3 != 3 * num_heads * HEAD_DIM:
        return False
    if not (1 <= b <= 65535 and s >= 1 and qkv.numel() < 2 ** 31):
        return False
    if not qkv.is_contiguous() or qkv.data_ptr() % 16 != 0:
        return False
    if not _lens_ok(qkv, seq_lens):
        return False
    native.require()
    return True


def _lens32(seq_lens: Optional[Tensor]) -> Optional[Tensor]:
    if seq_lens is None:
        return None
    return seq_lens.to(torch.int32).contiguous()  # a device op: no sync


def forward(qkv: Tensor, num_heads: int,
            seq_lens: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """``(out, lse)``; the caller has asked :func:`kernels_apply`."""
    b, s, h3 = qkv.shape
    out = qkv.new_empty(b, s, h3 // 3)
    lse = qkv.new_empty(b, num_heads, s, dtype=torch.float32)
    native.lib().attention_forward(qkv, _lens32(seq_lens), num_heads, out,
                                   lse)
    return out, lse


def backward(dout: Tensor, qkv: Tensor, out: Tensor, lse: Tensor,
             seq_lens: Optional[Tensor], num_heads: int) -> Tensor:
    """``dqkv``. ``dout`` is contiguous and 16-byte aligned, as ``out`` is."""
    dqkv = torch.empty_like(qkv)
    native.lib().attention_backward(dout, qkv, out, lse, _lens32(seq_lens),
                                    num_heads, dqkv)
    return dqkv


def reference(qkv: Tensor, num_heads: int,
              seq_lens: Optional[Tensor] = None) -> Tensor:
    """The same attention in torch ops, differentiable: SDPA with a key mask
    made from ``seq_lens``, padded rows zeroed going in (so that nothing
    stored there counts) and coming out."""
    b, s, h3 = qkv.shape
    h = h3 // 3
    valid = None
    if seq_lens is not None:
        pos = torch.arange(s, device=qkv.device)
        valid = pos[None, :] < seq_lens.clamp(0, s)[:, None]  # (B, S)
        qkv = torch.where(valid[:, :, None], qkv, qkv.new_zeros(()))
    q, k, v = (t.transpose(1, 2) for t in
               qkv.view(b, s, 3, num_heads, h // num_heads).unbind(2))
    if valid is None:
        y = F.scaled_dot_product_attention(q, k, v)
    else:
        # a padded query attends every key: finite, and zeroed below
        mask = valid[:, None, None, :] | ~valid[:, None, :, None]
        y = F.scaled_dot_product_attention(q, k, v, attn_mask=mask)
    y = y.transpose(1, 2).reshape(b, s, h)
    if valid is not None:
        y = torch.where(valid[:, :, None], y, y.new_zeros(()))
    return y
