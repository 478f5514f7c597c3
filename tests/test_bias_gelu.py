"""``contrib.FusedBiasGELU`` and BERT's use of it where no kernel runs: on
the CPU it is the torch chain, bit for bit."""

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from bagua_amd.contrib import FusedBiasGELU
from bagua_amd.models.bert import BertForPretrainingShape, bert_tiny


@pytest.mark.parametrize("form", ["none", "tanh"])
@pytest.mark.parametrize("with_bias", [True, False])
def test_module_is_the_torch_chain(form, with_bias):
    gen = torch.Generator().manual_seed(11)
    g = torch.randn(5, 24, generator=gen)
    outs = []
    for fused in (True, False):
        h = torch.randn(5, 24, generator=gen.manual_seed(12)).requires_grad_()
        b = torch.randn(24, generator=gen).requires_grad_()
        if not with_bias:
            a = (FusedBiasGELU(approximate=form)(h) if fused
                 else nn.GELU(approximate=form)(h))
        else:
            a = (FusedBiasGELU(approximate=form)(h, b) if fused
                 else F.gelu(h + b, approximate=form))
        outs.append((a,) + torch.autograd.grad(a, [h, b][:1 + with_bias], g))
    for got, want in zip(*outs):
        assert torch.equal(got, want)


def test_bert_tiny_is_the_parents_model(monkeypatch):
    torch.manual_seed(0)
    model = bert_tiny().eval()
    ids = torch.randint(0, 1024, (2, 16))
    outs = {}
    for flag in (True, False):
        monkeypatch.setattr(BertForPretrainingShape, "fuse_bias_gelu", flag)
        with torch.no_grad():
            outs[flag] = model(ids)
    for got, want in zip(outs[True], outs[False]):
        assert torch.equal(got, want)
    # the activation has no parameters: the keys of the nn.GELU model
    keys = list(model.state_dict())
    for layer in model.layers:
        assert isinstance(layer.mlp[1], FusedBiasGELU)
        layer.mlp[1] = nn.GELU()
    assert list(model.state_dict()) == keys
    assert "layers.0.mlp.0.bias" in keys
