"""``SyncBatchNorm(x, residual=z, relu=True)`` and the ResNet wiring on the
CPU, where the kernels decline: the same torch ops in the same order as the
unfused composition, so everything is bitwise equal. World size 1."""

import os
import socket

import pytest
import torch

from bagua_amd.contrib import SyncBatchNorm
from bagua_amd.models import resnet


@pytest.fixture(scope="module", autouse=True)
def _world_of_one():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    for key, value in (("WORLD_SIZE", "1"), ("RANK", "0"),
                       ("LOCAL_RANK", "0"), ("MASTER_ADDR", "127.0.0.1"),
                       ("MASTER_PORT", str(port))):
        os.environ.setdefault(key, value)
    import bagua_amd

    bagua_amd.init_process_group()


def _step(fused, with_residual):
    gen = torch.Generator().manual_seed(5)
    x, z, g = (torch.randn(4, 6, 5, 3, generator=gen) for _ in range(3))
    x.requires_grad_()
    z.requires_grad_()
    bn = SyncBatchNorm(6)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(6, generator=gen) + 0.5)
        bn.bias.copy_(torch.rand(6, generator=gen) - 0.5)
    if fused:
        y = bn(x, residual=z if with_residual else None, relu=True)
    else:
        y = torch.relu(bn(x) + z if with_residual else bn(x))
    leaves = [x, bn.weight, bn.bias] + ([z] if with_residual else [])
    return [y.detach(), bn.running_mean, bn.running_var,
            *torch.autograd.grad(y, leaves, g)]


@pytest.mark.parametrize("with_residual", [False, True])
def test_relu_keyword_is_the_unfused_composition_bitwise(with_residual):
    for a, b in zip(_step(True, with_residual), _step(False, with_residual)):
        assert torch.equal(a, b)


def test_residual_needs_relu_and_the_inputs_shape():
    bn, x = SyncBatchNorm(6), torch.randn(4, 6, 5, 3)
    with pytest.raises(ValueError):
        bn(x, residual=torch.randn(4, 6, 5, 3))
    with pytest.raises(ValueError):
        bn(x, residual=torch.randn(4, 6, 5, 1), relu=True)
    with pytest.raises(ValueError):
        bn(x, residual=torch.randn(4, 6, 5, 3).double(), relu=True)


def test_resnet18_same_bits_with_and_without_fuse_bn_act(monkeypatch):
    results = []
    for fuse in (True, False):
        monkeypatch.setattr(resnet.ResNet, "fuse_bn_act", fuse)
        torch.manual_seed(11)
        model = SyncBatchNorm.convert_sync_batchnorm(
            resnet.resnet18(num_classes=10))
        out = model(torch.randn(2, 3, 32, 32))
        out.square().sum().backward()
        results.append([out.detach()] + [p.grad for p in model.parameters()])
    assert len(results[0]) == len(results[1]) > 60
    for a, b in zip(*results):
        assert torch.equal(a, b)
