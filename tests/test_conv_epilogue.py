"""Fused conv epilogue (bagua_amd/ops/conv_epilogue.py), CPU side: the
torch implementation against the stock composition, VGG's fused walk
against its plain Sequential, and which inputs keep the stock path."""

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from bagua_amd.models import vgg as vgg_mod
from bagua_amd.models import vgg11, vgg16
from bagua_amd.ops import conv_epilogue


def _stock(x, b, pool):
    out = F.relu(x + b.view(1, -1, 1, 1))
    return F.max_pool2d(out, 2, 2) if pool else out


def _inputs(dtype, channels_last):
    gen = torch.Generator().manual_seed(7)
    x = torch.randn(2, 8, 4, 6, generator=gen)
    b = torch.randn(8, generator=gen)
    # windows (n, c, 0:2, 0:2), with biases that keep x + b exact: exact
    # positive ties (first, then a later position), all equal, all-zero
    # and all-negative
    b[:5] = torch.tensor([0.5, -0.25, 1.0, 2.0, -1.0])
    x[0, 0, 0:2, 0:2] = torch.tensor([[1.5, 1.5], [0.25, 1.5]]) - b[0]
    x[0, 1, 0:2, 0:2] = torch.tensor([[0.5, 2.0], [2.0, 2.0]]) - b[1]
    x[0, 2, 0:2, 0:2] = 3.0 - b[2]
    x[0, 3, 0:2, 0:2] = -b[3]
    x[0, 4, 0:2, 0:2] = -5.0
    x, b = x.to(dtype), b.to(dtype)
    if channels_last:
        x = x.contiguous(memory_format=torch.channels_last)
    return x, b


@pytest.mark.parametrize("channels_last", [False, True])
@pytest.mark.parametrize("pool", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_torch_path_equals_stock(dtype, pool, channels_last):
    x, b = _inputs(dtype, channels_last)
    x0, b0 = x.clone().requires_grad_(), b.clone().requires_grad_()
    x1, b1 = x.clone().requires_grad_(), b.clone().requires_grad_()
    out = conv_epilogue.conv_bias_relu(x0 * 1, b0, pool)
    ref = _stock(x1, b1, pool)
    assert out.dtype == dtype and torch.equal(out, ref)
    if pool:  # the prepared windows did what they were prepared for
        assert out[0, 3, 0, 0] == 0 and out[0, 4, 0, 0] == 0
        assert out[0, 2, 0, 0] == 3.0
    g = torch.randn(ref.shape, generator=torch.Generator().manual_seed(8))
    g = g.to(dtype)
    out.backward(g)
    ref.backward(g)
    assert torch.equal(x0.grad, x1.grad)
    assert torch.equal(b0.grad, b1.grad)
    if pool:
        # first maximum wins a tie; zero and negative windows pass nothing
        assert x0.grad[0, 0, 0, 0] == g[0, 0, 0, 0]
        assert x0.grad[0, 1, 0, 1] == g[0, 1, 0, 0]
        assert x0.grad[0, 2, 0, 0] == g[0, 2, 0, 0]
        assert not x0.grad[0, 3, 0:2, 0:2].any()
        assert not x0.grad[0, 4, 0:2, 0:2].any()


def test_torch_bias_grad_switch_and_no_grad():
    x, b = _inputs(torch.float32, True)
    b0 = b.clone().requires_grad_()
    out = conv_epilogue.conv_bias_relu(
        x.clone().requires_grad_() * 1, b0, True, torch_bias_grad=True)
    out.sum().backward()
    b1 = b.clone().requires_grad_()
    _stock(x, b1, True).sum().backward()
    assert torch.equal(b0.grad, b1.grad)
    with torch.no_grad():
        y = x.clone()
        assert conv_epilogue.conv_bias_relu(y, b) is y
        assert torch.equal(y, _stock(x, b, False))


def test_vgg16_parameters_unchanged():
    model = vgg16()
    names = [n for n, _ in model.named_parameters()]
    convs = [0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28]
    expect = []
    for i in convs:
        expect += ["features.%d.weight" % i, "features.%d.bias" % i]
    for i in (0, 3, 6):
        expect += ["classifier.%d.weight" % i, "classifier.%d.bias" % i]
    assert names == expect
    assert list(model.state_dict().keys()) == expect
    assert isinstance(model.features, nn.Sequential)
    assert len(model.features) == 31
    kinds = "".join("C" if isinstance(m, nn.Conv2d) else
                    "R" if isinstance(m, nn.ReLU) else "M"
                    for m in model.features)
    assert kinds == "CRCRM" * 2 + "CRCRCRM" * 3
    assert vgg_mod.VGG.torch_bias_grad is False


def _always(x, conv, pool):
    return True


@pytest.mark.parametrize("batch_norm", [False, True])
def test_vgg_fused_walk_equals_sequential(monkeypatch, batch_norm):
    """Forward and backward through VGG.forward equal the plain Sequential;
    with the eligibility test forced, the walk really goes through the
    fused function (its torch implementation here)."""
    torch.manual_seed(3)
    model = vgg11(num_classes=10, batch_norm=batch_norm).eval()
    x = torch.randn(2, 3, 32, 32)

    def plain(inp):
        out = model.avgpool(model.features(inp))
        return model.classifier(torch.flatten(out, 1))

    def grads(fn):
        model.zero_grad()
        inp = x.clone().requires_grad_()
        out = fn(inp)
        out.square().sum().backward()
        return [out.detach(), inp.grad] + [p.grad.clone()
                                           for p in model.parameters()]

    ref = grads(plain)
    for a, r in zip(grads(model), ref):  # CPU: nothing is eligible
        assert torch.equal(a, r)

    calls = []
    real = conv_epilogue.conv_bias_relu

    def spy(conv_out, bias, pool=False, torch_bias_grad=False):
        calls.append(pool)
        return real(conv_out, bias, pool, torch_bias_grad)

    def split_bias(inp):
        # the Sequential with every conv bias added after a bias-free
        # convolution, as torch-ROCm does it (the CPU convolution adds
        # the bias inside and rounds differently)
        out = inp
        for m in model.features:
            if isinstance(m, nn.Conv2d):
                out = F.conv2d(out, m.weight, None, m.stride, m.padding)
                out = out + m.bias.view(1, -1, 1, 1)
            else:
                out = m(out)
        return model.classifier(torch.flatten(model.avgpool(out), 1))

    if not batch_norm:  # with BN nothing is fused: the modules run
        ref = grads(split_bias)
    monkeypatch.setattr(conv_epilogue, "conv_eligible", _always)
    monkeypatch.setattr(conv_epilogue, "conv_bias_relu", spy)
    got = grads(model)
    # vgg11: conv-relu-pool x2, then (conv-relu, conv-relu-pool) x3
    assert calls == ([] if batch_norm
                     else [True, True, False, True, False, True,
                           False, True])
    for a, r in zip(got, ref):
        assert torch.equal(a, r)


def test_vgg_hooked_module_keeps_stock_path(monkeypatch):
    model = vgg11(num_classes=10).eval()
    seen = []
    model.features[0].register_forward_hook(
        lambda m, i, o: seen.append(tuple(o.shape)))
    calls = []
    real = conv_epilogue.conv_bias_relu
    monkeypatch.setattr(conv_epilogue, "conv_eligible", _always)
    monkeypatch.setattr(
        conv_epilogue, "conv_bias_relu",
        lambda *a, **k: calls.append(1) or real(*a, **k))
    with torch.no_grad():
        model(torch.randn(1, 3, 32, 32))
    assert seen == [(1, 64, 32, 32)]
    assert len(calls) == 7  # every stage but the hooked one


def _fake_cuda(shape, dtype=torch.bfloat16, channels_last=True):
    """A meta tensor that reports is_cuda: conv_eligible reads only
    metadata, so the GPU-side decisions can be checked without one."""
    t = torch.empty(shape, dtype=dtype, device="meta")
    if channels_last:
        t = t.contiguous(memory_format=torch.channels_last)

    class Fake:
        is_cuda = True

        def __getattr__(self, name):
            return getattr(t, name)

    return Fake()


def _conv(cin, cout, dtype=torch.bfloat16, **kw):
    return nn.Conv2d(cin, cout, 3, padding=1, **kw).to(dtype)


def test_eligibility(monkeypatch):
    monkeypatch.setattr(conv_epilogue.native, "require", lambda: None)
    ok = conv_epilogue.conv_eligible
    x = _fake_cuda((2, 16, 6, 10))
    assert ok(x, _conv(16, 64), False) and ok(x, _conv(16, 64), True)
    # the image itself: 3 input channels are fine, it is C of the output
    assert ok(_fake_cuda((2, 3, 8, 8)), _conv(3, 64), True)
    # odd H or W: no fused pooling, the unpooled epilogue still applies
    for shape in ((2, 16, 5, 10), (2, 16, 6, 9)):
        assert not ok(_fake_cuda(shape), _conv(16, 64), True)
        assert ok(_fake_cuda(shape), _conv(16, 64), False)
    # C = 3 or any C that is no multiple of the 16-byte vector
    assert not ok(x, _conv(16, 3), False)
    assert not ok(x, _conv(16, 12), False)
    assert ok(_fake_cuda((2, 16, 6, 10), torch.float32),
              _conv(16, 12, torch.float32), False)
    # more channel vectors than a block has lanes
    assert not ok(x, _conv(16, 4096), False)
    # NCHW
    assert not ok(_fake_cuda((2, 16, 6, 10), channels_last=False),
                  _conv(16, 64), False)
    # mixed dtypes, unsupported dtype, no bias, CPU
    assert not ok(x, _conv(16, 64, torch.float32), False)
    assert not ok(_fake_cuda((2, 16, 6, 10), torch.float64),
                  _conv(16, 64, torch.float64), False)
    assert not ok(x, _conv(16, 64, bias=False), False)
    assert not ok(torch.empty(2, 16, 6, 10, dtype=torch.bfloat16).contiguous(
        memory_format=torch.channels_last), _conv(16, 64), False)
    # other padding modes are not the bias-free F.conv2d call
    assert not ok(x, _conv(16, 64, padding_mode="reflect"), False)
    # autocast on
    monkeypatch.setattr(torch, "is_autocast_enabled", lambda *a: True)
    assert not ok(x, _conv(16, 64), False)


def test_ineligible_function_inputs_take_torch_path():
    """The function itself declines the same cases (here all of them, on
    CPU) and still computes the stock result."""
    assert not conv_epilogue.kernels_apply(
        torch.zeros(1, 8, 2, 2), torch.zeros(8), False)
    gen = torch.Generator().manual_seed(5)
    for shape, dtype in (((1, 3, 5, 7), torch.float32),
                         ((2, 8, 3, 5), torch.bfloat16),
                         ((1, 4, 2, 2), torch.float64)):
        x = torch.randn(shape, generator=gen).to(dtype)
        b = torch.randn(shape[1], generator=gen).to(dtype)
        assert torch.equal(conv_epilogue.conv_bias_relu(x.clone(), b),
                           _stock(x, b, False))
