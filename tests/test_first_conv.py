"""ops/first_conv.py on the CPU: what `eligible` declines, read from
metadata alone, and that VGG16 still equals the plain Sequential where the
fused first stage does not apply."""

import torch
import torch.nn as nn

from bagua_amd.models.vgg import VGG, _CFGS
from bagua_amd.ops import first_conv


def _fake_cuda(shape, dtype=torch.bfloat16, channels_last=True,
               requires_grad=False):
    """A meta tensor that reports is_cuda: `eligible` reads only metadata,
    so the GPU-side decisions can be checked without one."""
    t = torch.empty(shape, dtype=dtype, device="meta")
    if channels_last:
        t = t.contiguous(memory_format=torch.channels_last)
    t.requires_grad_(requires_grad)

    class Fake:
        is_cuda = True

        def __getattr__(self, name):
            return getattr(t, name)

    return Fake()


def _conv(cin=3, cout=64, dtype=torch.bfloat16, **kw):
    kw.setdefault("padding", 1)
    return nn.Conv2d(cin, cout, 3, **kw).to(dtype)


def test_eligibility(monkeypatch):
    monkeypatch.setattr(first_conv.native, "require", lambda: None)
    ok = first_conv.eligible
    x = _fake_cuda((2, 3, 8, 10))
    assert ok(x, _conv())
    assert ok(_fake_cuda((1, 3, 1, 1)), _conv())
    # channels-last weights are taken through their strides
    assert ok(x, _conv().to(memory_format=torch.channels_last))
    # CPU tensor
    assert not ok(torch.empty(2, 3, 8, 10, dtype=torch.bfloat16).contiguous(
        memory_format=torch.channels_last), _conv())
    # f32, on either side
    assert not ok(_fake_cuda((2, 3, 8, 10), torch.float32),
                  _conv(dtype=torch.float32))
    assert not ok(x, _conv(dtype=torch.float32))
    # other shapes of the convolution
    assert not ok(_fake_cuda((2, 4, 8, 10)), _conv(4))
    assert not ok(x, _conv(cout=32))
    assert not ok(x, _conv(stride=2))
    assert not ok(x, _conv(padding=0))
    assert not ok(x, _conv(padding=2, dilation=2))
    assert not ok(x, _conv(padding_mode="reflect"))
    assert not ok(x, nn.Conv2d(3, 64, 5, padding=1).bfloat16())
    # an image that wants a gradient needs dx
    assert not ok(_fake_cuda((2, 3, 8, 10), requires_grad=True), _conv())
    # NCHW input
    assert not ok(_fake_cuda((2, 3, 8, 10), channels_last=False), _conv())
    # no bias
    assert not ok(x, _conv(bias=False))
    # N*H*W at 2^31
    assert not ok(_fake_cuda((2, 3, 2 ** 15, 2 ** 15)), _conv())
    assert ok(_fake_cuda((2, 3, 2 ** 15, 2 ** 15 - 1)), _conv())
    # autocast on
    monkeypatch.setattr(torch, "is_autocast_enabled", lambda *a: True)
    assert not ok(x, _conv())


def test_vgg16_on_cpu_equals_sequential():
    torch.manual_seed(4)
    # VGG16's features; the head stays small
    model = VGG(_CFGS["D"], num_classes=10).eval()
    x = torch.randn(2, 3, 32, 32)

    def plain(inp):
        out = model.avgpool(model.features(inp))
        return model.classifier(torch.flatten(out, 1))

    def grads(fn):
        model.zero_grad()
        out = fn(x)
        out.square().sum().backward()
        return [out.detach()] + [p.grad.clone() for p in model.parameters()]

    for a, r in zip(grads(model), grads(plain)):
        assert torch.equal(a, r)
