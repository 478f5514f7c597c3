"""BERT encoder for the SQuAD-shape decentralized benchmark
(BASELINE.json config: "BERT-Large SQuAD-shape Decentralized-SGD").

Plain transformer encoder matching BERT-Large dimensions (24 layers,
hidden 1024, 16 heads, ffn 4096) with a span-prediction head (start/end
logits) — the training *shape* of SQuAD finetuning on synthetic data.
"""

import math
from dataclasses import dataclass

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..contrib.add_layernorm import FusedDropoutAddLayerNorm
from ..contrib.bias_gelu import FusedBiasGELU
from ..contrib.self_attention import PackedSelfAttention


@dataclass
class BertConfig:
    vocab_size: int = 30522
    hidden_size: int = 1024
    num_layers: int = 24
    num_heads: int = 16
    intermediate_size: int = 4096
    max_position: int = 512
    dropout: float = 0.1


def _has_hooks(m: nn.Module) -> bool:
    return bool(m._forward_hooks or m._forward_pre_hooks
                or m._backward_hooks or m._backward_pre_hooks)


def _fused(x, *modules, flag="fuse_add_ln") -> bool:
    """Whether a fused path of ``BertForPretrainingShape`` is taken (see its
    ``fuse_add_ln``, ``fuse_bias_gelu`` and ``fuse_attention``): the flag is
    on, on the GPU, and
    nobody has hooked a module whose call the fused path leaves out."""
    return (getattr(BertForPretrainingShape, flag) and x.is_cuda
            and not any(_has_hooks(m) for m in modules))


def _add_ln(ln, x, inp, lin, drop):
    """``ln(x + drop(lin(inp)))`` with the bias of ``lin``, the dropout and
    the add inside the norm: the Linear runs without its bias."""
    return ln(x, F.linear(inp, lin.weight), lin.bias,
              drop.p if drop.training else 0.0)


class _MlpGELU(FusedBiasGELU):
    """``mlp[1]``. The fused path hands it the first Linear's bias; called
    without one, as ``nn.Sequential`` calls it, the bias is already in ``h``
    and this is ``nn.GELU.forward``, the modules one by one."""

    def forward(self, h, bias=None):
        return super().forward(h, bias, kernels=bias is not None)


class BertSelfAttention(nn.Module):
    def __init__(self, cfg: BertConfig):
        super().__init__()
        self.num_heads = cfg.num_heads
        self.head_dim = cfg.hidden_size // cfg.num_heads
        self.qkv = nn.Linear(cfg.hidden_size, 3 * cfg.hidden_size)
        self.out = nn.Linear(cfg.hidden_size, cfg.hidden_size)
        self.dropout = nn.Dropout(cfg.dropout)
        self.core = PackedSelfAttention(cfg.num_heads)  # no parameters

    def context(self, x, seq_lens=None):
        """The attention output in front of the ``out`` projection. With
        ``seq_lens`` (``(B,)`` integers on the device of ``x``) keys at or
        behind a sequence's length are not attended and its rows there come
        out as zeros."""
        B, S, H = x.shape
        if seq_lens is not None or _fused(x, flag="fuse_attention"):
            return self.core(self.qkv(x), seq_lens)
        qkv = self.qkv(x).view(B, S, 3, self.num_heads, self.head_dim)
        q, k, v = qkv.unbind(2)
        q = q.transpose(1, 2)  # B, h, S, d
        k = k.transpose(1, 2)
        v = v.transpose(1, 2)
        # scaled_dot_product_attention lowers to the ROCm fused path on GPU
        y = torch.nn.functional.scaled_dot_product_attention(q, k, v)
        return y.transpose(1, 2).reshape(B, S, H)

    def forward(self, x, seq_lens=None):
        return self.dropout(self.out(self.context(x, seq_lens)))


class BertLayer(nn.Module):
    def __init__(self, cfg: BertConfig):
        super().__init__()
        self.attn = BertSelfAttention(cfg)
        self.ln1 = FusedDropoutAddLayerNorm(cfg.hidden_size)
        self.mlp = nn.Sequential(
            nn.Linear(cfg.hidden_size, cfg.intermediate_size),
            _MlpGELU(),
            nn.Linear(cfg.intermediate_size, cfg.hidden_size),
            nn.Dropout(cfg.dropout),
        )
        self.ln2 = FusedDropoutAddLayerNorm(cfg.hidden_size)

    def forward(self, x, seq_lens=None):
        attn, mlp = self.attn, self.mlp
        if _fused(x, attn, attn.out, attn.dropout, self.ln1):
            x = _add_ln(self.ln1, x, attn.context(x, seq_lens), attn.out,
                        attn.dropout)
        elif seq_lens is None:
            x = self.ln1(x + attn(x), kernels=False)
        else:
            x = self.ln1(x + attn(x, seq_lens), kernels=False)
        gelu = _fused(x, mlp, mlp[0], mlp[1], flag="fuse_bias_gelu")
        add_ln = _fused(x, mlp, mlp[2], mlp[3], self.ln2)
        if not (gelu or add_ln):
            return self.ln2(x + mlp(x), kernels=False)
        # nobody has hooked mlp itself: its modules by hand
        if gelu:  # the Linear without its bias, which goes to the activation
            mid = mlp[1](F.linear(x, mlp[0].weight), mlp[0].bias)
        else:
            mid = mlp[1](mlp[0](x))
        if add_ln:
            return _add_ln(self.ln2, x, mid, mlp[2], mlp[3])
        return self.ln2(x + mlp[3](mlp[2](mid)), kernels=False)


class BertForPretrainingShape(nn.Module):
    """BERT encoder + SQuAD span head; input is token ids, output is
    (start_logits, end_logits)."""

    # Every sub-layer's tail, LayerNorm(x + Dropout(Linear(...))), and the
    # embedding norm run in the kernels of FusedDropoutAddLayerNorm: the
    # Linear's bias, the dropout and the add happen in f32 inside the norm's
    # one pass each way, with the branch in its own dtype (GPU only;
    # elsewhere the choice changes nothing). False runs the modules one by
    # one, the norms as nn.LayerNorm.
    fuse_add_ln = True

    # The middle of every MLP, GELU(Linear(x)), runs in the kernels of
    # FusedBiasGELU: the first Linear runs without its bias, which is added
    # in f32 inside the activation's one pass each way, and the backward pass
    # leaves the bias gradient with it, so that no separate pass over the
    # gradient sums it (GPU only; elsewhere the choice changes nothing).
    # False runs the modules one by one, the activation as nn.GELU.
    # Independent of fuse_add_ln.
    fuse_bias_gelu = True

    # Attention without lengths runs in the kernels of PackedSelfAttention,
    # which read the qkv Linear's output where it lies and write (B, S, H)
    # and one packed gradient, in place of scaled_dot_product_attention
    # between transposed views and a copy back (GPU only, where the kernels
    # take the shape: f16 or bf16, head_dim 64; elsewhere the choice changes
    # nothing). False runs that torch chain. With seq_lens given, attention
    # is PackedSelfAttention whatever this says: the chain has no lengths.
    # Independent of the two above.
    fuse_attention = True

    def __init__(self, cfg: BertConfig = None):
        super().__init__()
        cfg = cfg or BertConfig()
        self.cfg = cfg
        self.tok_emb = nn.Embedding(cfg.vocab_size, cfg.hidden_size)
        self.pos_emb = nn.Embedding(cfg.max_position, cfg.hidden_size)
        self.emb_ln = FusedDropoutAddLayerNorm(cfg.hidden_size)
        self.layers = nn.ModuleList(
            [BertLayer(cfg) for _ in range(cfg.num_layers)])
        self.qa_head = nn.Linear(cfg.hidden_size, 2)
        self.apply(self._init)

    def _init(self, m):
        if isinstance(m, (nn.Linear, nn.Embedding)):
            nn.init.normal_(m.weight, std=0.02 / math.sqrt(2))
            if isinstance(m, nn.Linear) and m.bias is not None:
                nn.init.zeros_(m.bias)

    def forward(self, input_ids, seq_lens=None):
        """``seq_lens``: None, or ``(B,)`` integers on the device of
        ``input_ids``: sequence ``b`` is ``input_ids[b, :seq_lens[b]]`` and
        what lies behind is padding, which no valid position attends. Logits
        at padded positions mean nothing."""
        B, S = input_ids.shape
        pos = torch.arange(S, device=input_ids.device).unsqueeze(0)
        x = self.tok_emb(input_ids) + self.pos_emb(pos)
        x = self.emb_ln(x, kernels=_fused(x, self.emb_ln))
        for layer in self.layers:
            x = layer(x) if seq_lens is None else layer(x, seq_lens)
        logits = self.qa_head(x)  # B, S, 2
        return logits[..., 0], logits[..., 1]


def bert_large():
    return BertForPretrainingShape(BertConfig())


def bert_tiny():
    """4-layer miniature for CPU tests."""
    return BertForPretrainingShape(BertConfig(
        vocab_size=1024, hidden_size=128, num_layers=4, num_heads=4,
        intermediate_size=256, max_position=128))
