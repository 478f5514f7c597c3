"""``seq_lens`` through BERT and ``contrib.PackedSelfAttention`` in its torch
form, on the CPU in float64: padding changes nothing in front of a length."""

import pytest
import torch

from bagua_amd.contrib import PackedSelfAttention
from bagua_amd.models.bert import BertConfig, BertForPretrainingShape

L, S = 5, 9


def _step(model, ids, lens, rows):
    model.zero_grad()
    start, end = model(ids, lens)
    logits = torch.stack([start[0, :rows], end[0, :rows]])
    (logits.square().sum() + logits.sum()).backward()
    return logits.detach(), {n: p.grad.clone()
                             for n, p in model.named_parameters()}


@pytest.mark.parametrize("fill", [0, 7])
def test_padding_invariance(fill):
    torch.manual_seed(1)
    model = BertForPretrainingShape(BertConfig(
        vocab_size=64, hidden_size=32, num_layers=2, num_heads=2,
        intermediate_size=64, max_position=16, dropout=0.0)).double()
    ids = torch.randint(0, 64, (1, L))
    padded = torch.cat([ids, torch.full((1, S - L), fill)], dim=1)
    alone, grads_alone = _step(model, ids, None, L)
    got, grads = _step(model, padded, torch.tensor([L]), L)
    assert torch.allclose(got, alone, rtol=0, atol=1e-12)
    for n, g in grads_alone.items():
        assert torch.allclose(grads[n], g, rtol=0, atol=1e-11), n


def test_packed_self_attention_gradcheck():
    gen = torch.Generator().manual_seed(2)
    qkv = torch.randn(3, 4, 3 * 2 * 3, generator=gen,
                      dtype=torch.float64).requires_grad_()
    lens = torch.tensor([4, 2, 0])
    attn = PackedSelfAttention(2)
    out = attn(qkv, lens)
    assert not out[1, 2:].any() and not out[2].any()
    assert torch.autograd.gradcheck(lambda t: attn(t, lens), (qkv,))
    grad, = torch.autograd.grad(attn(qkv, lens).sum(), qkv)
    assert not grad[1, 2:].any() and not grad[2].any()
