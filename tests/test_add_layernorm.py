"""``contrib.FusedDropoutAddLayerNorm`` and BERT's use of it where no kernel
runs: the CPU chain is the written-out torch ops, bit for bit."""

import pytest
import torch
import torch.nn.functional as F

from bagua_amd.contrib import FusedDropoutAddLayerNorm
from bagua_amd.models.bert import BertForPretrainingShape, bert_tiny

LAYER0_KEYS = [
    "layers.0.attn.qkv.weight", "layers.0.attn.qkv.bias",
    "layers.0.attn.out.weight", "layers.0.attn.out.bias",
    "layers.0.ln1.weight", "layers.0.ln1.bias",
    "layers.0.mlp.0.weight", "layers.0.mlp.0.bias",
    "layers.0.mlp.2.weight", "layers.0.mlp.2.bias",
    "layers.0.ln2.weight", "layers.0.ln2.bias",
]
OTHER_KEYS = ["tok_emb.weight", "pos_emb.weight", "emb_ln.weight",
              "emb_ln.bias", "qa_head.weight", "qa_head.bias"]


@pytest.mark.parametrize("branch,bias,p", [
    (False, False, 0.0), (True, False, 0.0), (True, True, 0.0),
    (True, False, 0.3), (True, True, 0.3)])
def test_module_is_the_torch_chain_on_cpu(branch, bias, p):
    gen = torch.Generator().manual_seed(11)
    ln = FusedDropoutAddLayerNorm(24)
    with torch.no_grad():
        ln.weight.add_(torch.randn(24, generator=gen))
        ln.bias.add_(torch.randn(24, generator=gen))
    data = [torch.randn(3, 5, 24, generator=gen), None, None]
    if branch:
        data[1] = torch.randn(3, 5, 24, generator=gen)
    if bias:
        data[2] = torch.randn(24, generator=gen)
    g = torch.randn(3, 5, 24, generator=gen)
    results = []
    for fused in (True, False):
        x, h, b = (None if t is None else t.clone().requires_grad_()
                   for t in data)
        torch.manual_seed(5)
        if fused:
            y = ln(x, h, b, p)
        else:
            s = x
            if h is not None:
                s = x + F.dropout(h if b is None else h + b, p, True)
            y = F.layer_norm(s, (24,), ln.weight, ln.bias, ln.eps)
        leaves = [t for t in (x, h, b, ln.weight, ln.bias) if t is not None]
        results.append([y.detach()] + list(torch.autograd.grad(y, leaves, g)))
    for got, want in zip(*results):
        assert torch.equal(got, want)


def test_bert_tiny_same_bits_with_and_without_the_flag(monkeypatch):
    torch.manual_seed(0)
    model = bert_tiny().train()
    ids = torch.randint(0, 1024, (2, 16))
    results = []
    for flag in (True, False):
        monkeypatch.setattr(BertForPretrainingShape, "fuse_add_ln", flag)
        model.zero_grad()
        torch.manual_seed(3)
        start, end = model(ids)
        (start.square().sum() + end.sum()).backward()
        results.append([start.detach(), end.detach()]
                       + [p.grad.clone() for p in model.parameters()])
    for got, want in zip(*results):
        assert torch.equal(got, want)


def test_bert_tiny_state_dict_keys_unchanged():
    keys = list(bert_tiny().state_dict())
    want = OTHER_KEYS[:4]
    for i in range(4):
        want += [k.replace("layers.0.", "layers.%d." % i)
                 for k in LAYER0_KEYS]
    assert keys == want + OTHER_KEYS[4:]
