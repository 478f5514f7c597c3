"""Off the GPU nothing changes: ``ops.batchnorm.kernels_apply`` declines
CPU tensors without loading the extension, and ``SyncBatchNorm`` computes,
bit for bit, the formulae it always did."""

import pytest
import torch

from bagua_amd.contrib import sync_batchnorm
from bagua_amd.ops import batchnorm as bn_ops

EPS, MOMENTUM = 1e-5, 0.1


def test_kernels_decline_cpu_without_the_extension(monkeypatch):
    def boom():
        raise AssertionError("the extension was asked for")

    monkeypatch.setattr(bn_ops.native, "require", boom)
    monkeypatch.setattr(bn_ops.native, "lib", boom)
    x = torch.randn(2, 8, 3, 3).contiguous(memory_format=torch.channels_last)
    w = torch.ones(8)
    assert not bn_ops.kernels_apply(x, w, w, w, w, MOMENTUM)
    assert not bn_ops.kernels_apply(x.bfloat16(), None, None, None, None,
                                    MOMENTUM)


def _formulae(x, g, w, b, rmean, rvar):
    """Forward and backward of one rank, as contrib/sync_batchnorm.py has
    written them since before the kernels."""
    c = x.shape[1]
    dims = [0] + list(range(2, x.dim()))
    shape = [1, c] + [1] * (x.dim() - 2)
    count = torch.tensor(float(x.numel() // c))
    mean = x.float().sum(dim=dims) / count
    var = (x.float() ** 2).sum(dim=dims) / count - mean ** 2
    invstd = torch.rsqrt(var + EPS)
    rmean = rmean.clone().mul_(1 - MOMENTUM).add_(mean, alpha=MOMENTUM)
    rvar = rvar.clone().mul_(1 - MOMENTUM).add_(var * count / (count - 1),
                                                alpha=MOMENTUM)
    y = ((x.float() - mean.view(shape)) * invstd.view(shape)
         * w.view(shape) + b.view(shape))
    xmu = x.float() - mean.view(shape)
    sum_dy = g.sum(dim=dims)
    sum_dy_xmu = (g * xmu).sum(dim=dims)
    dx = ((g - sum_dy.view(shape) / count
           - xmu * invstd.view(shape) ** 2 * sum_dy_xmu.view(shape) / count)
          * invstd.view(shape) * w.view(shape))
    return dict(y=y, dx=dx, gw=sum_dy_xmu * invstd, gb=sum_dy, rmean=rmean,
                rvar=rvar)


@pytest.mark.parametrize("shape", [(4, 6, 5, 3), (7, 5)])
def test_cpu_module_is_bitwise_the_old_formulae(shape, monkeypatch):
    # world size 1: the SUM-allreduce leaves its vector as it is
    monkeypatch.setattr(sync_batchnorm, "allreduce_inplace",
                        lambda tensor, op=None: None)
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(shape, generator=gen) * 1.5 + 0.25
    g = torch.randn(shape, generator=gen)
    bn = sync_batchnorm.SyncBatchNorm(shape[1], eps=EPS, momentum=MOMENTUM)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(shape[1], generator=gen) + 0.5)
        bn.bias.copy_(torch.randn(shape[1], generator=gen))
        bn.running_mean.copy_(torch.randn(shape[1], generator=gen))
    want = _formulae(x, g, bn.weight.detach(), bn.bias.detach(),
                     bn.running_mean, bn.running_var)
    xl = x.clone().requires_grad_()
    y = bn(xl)
    y.backward(g)
    got = dict(y=y.detach(), dx=xl.grad, gw=bn.weight.grad, gb=bn.bias.grad,
               rmean=bn.running_mean, rvar=bn.running_var)
    for key, ref in want.items():
        assert torch.equal(got[key], ref), key
