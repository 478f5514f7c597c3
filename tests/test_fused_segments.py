"""FusedSGD reads gradients where they live: no flat gradient copy, and
at world size 1 no re-pin of the gradients into a bucket nobody reads."""

import copy
import os

import pytest
import torch

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")


def _old_cpu_sgd(ref, flat_g, m, initialized, lr, mu, damp, wd, nesterov):
    """The CPU step as it was when the optimizer kept a flat gradient
    (zeros where a parameter had no grad). Updates ref and m in place."""
    grad = flat_g.float() if ref.dtype != flat_g.dtype else flat_g
    if wd != 0:
        grad = grad.add(ref, alpha=wd)
    if mu != 0:
        if initialized:
            m.mul_(mu).add_(grad, alpha=1 - damp)
        else:
            m.copy_(grad)
        grad = grad.add(m, alpha=mu) if nesterov else m
    ref.add_(grad, alpha=-lr)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["f32", "bf16_master"])
@pytest.mark.parametrize("nesterov", [False, True])
def test_cpu_step_with_a_missing_grad(dtype, nesterov):
    from bagua_amd.contrib import FusedSGD

    torch.manual_seed(11)
    lr, mu, damp, wd = 0.05, 0.9, 0.0, 1e-2
    shapes = [(5, 3), (7,), (2, 4), (9,)]
    unused = 2   # never takes part in the loss: its grad stays None
    params = [torch.nn.Parameter(torch.randn(s).to(dtype)) for s in shapes]
    ref = torch.cat([p.detach().reshape(-1) for p in params]).float()
    if dtype == torch.float32:
        ref = ref.clone()
    m = torch.zeros_like(ref)
    opt = FusedSGD(params, lr=lr, momentum=mu, dampening=damp,
                   weight_decay=wd, nesterov=nesterov)
    assert "flat_g" not in opt._flat[0]
    for step in range(5):
        x = [torch.randn(s).to(dtype) for s in shapes]
        opt.zero_grad()
        loss = sum((p * xi).sum() * (k + 1)
                   for k, (p, xi) in enumerate(zip(params, x))
                   if k != unused)
        loss.backward()
        assert params[unused].grad is None
        # d loss / d p_k = (k + 1) * x_k, rounded to the parameter dtype
        flat_g = torch.cat([
            (torch.zeros(s) if k == unused
             else (xi.float() * (k + 1))).to(dtype).reshape(-1)
            for k, (s, xi) in enumerate(zip(shapes, x))])
        _old_cpu_sgd(ref, flat_g, m, step > 0, lr, mu, damp, wd, nesterov)
        opt.step()
        got = torch.cat([p.detach().reshape(-1) for p in params])
        assert torch.equal(got, ref.to(dtype)), "step %d" % step
        assert torch.equal(opt._flat[0]["momentum_buffer"], m)
    if dtype == torch.bfloat16:
        assert torch.equal(opt._flat[0]["master"], ref)


def _setup_env():
    os.environ.setdefault("WORLD_SIZE", "1")
    os.environ.setdefault("RANK", "0")
    os.environ.setdefault("LOCAL_RANK", "0")
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29593")


def _mlp():
    torch.manual_seed(21)
    return torch.nn.Sequential(
        torch.nn.Linear(24, 40), torch.nn.ReLU(),
        torch.nn.Linear(40, 17), torch.nn.ReLU(),
        torch.nn.Linear(17, 8)).cuda().bfloat16()


def _in_bucket(ddp, grad):
    for b in ddp.inner.bagua_buckets:
        flat = b._flat
        lo = flat.data_ptr()
        if lo <= grad.data_ptr() < lo + flat.numel() * flat.element_size():
            return True
    return False


def _train(model, optimizer, forward, steps=3):
    gen = torch.Generator(device="cuda").manual_seed(5)
    for _ in range(steps):
        x = torch.randn(16, 24, device="cuda", generator=gen).bfloat16()
        optimizer.zero_grad()
        forward(x).float().square().mean().backward()
        optimizer.step()
    torch.cuda.synchronize()


@pytest.mark.gpu
@requires_gpu
def test_world1_grads_stay_out_of_the_unread_bucket():
    _setup_env()
    import bagua_amd
    from bagua_amd.contrib import FusedSGD
    from bagua_amd.parallel.algorithms import GlobalAlgorithmRegistry

    torch.cuda.set_device(0)
    bagua_amd.init_process_group()

    plain = _mlp()
    wrapped = copy.deepcopy(plain)
    compressed = copy.deepcopy(plain)

    # plain FusedSGD, no wrapper
    opt_plain = FusedSGD(plain.parameters(), lr=0.05, momentum=0.9)
    _train(plain, opt_plain, plain)

    # gradient_allreduce at world size 1: nothing reads the bucket
    opt = FusedSGD(wrapped.parameters(), lr=0.05, momentum=0.9)
    ddp = bagua_amd.DistributedDataParallel(
        wrapped, optimizers=[opt],
        algorithm=GlobalAlgorithmRegistry.get("gradient_allreduce")())
    assert all(t.bucket_unread for b in ddp.inner.bagua_buckets
               for t in b.tensors)
    _train(wrapped, opt, ddp)
    for name, p in wrapped.named_parameters():
        assert p.grad is not None
        assert not _in_bucket(ddp, p.grad), name + ".grad is a bucket view"
    for (name, p), q in zip(wrapped.named_parameters(), plain.parameters()):
        assert torch.equal(p.detach().view(torch.int16),
                           q.detach().view(torch.int16)), name
    assert torch.equal(opt._flat[0]["master"], opt_plain._flat[0]["master"])

    # bytegrad quantizes the bucket even at world size 1: still re-pinned
    opt_c = FusedSGD(compressed.parameters(), lr=0.05, momentum=0.9)
    ddp_c = bagua_amd.DistributedDataParallel(
        compressed, optimizers=[opt_c],
        algorithm=GlobalAlgorithmRegistry.get("bytegrad")())
    assert not any(t.bucket_unread for b in ddp_c.inner.bagua_buckets
                   for t in b.tensors)
    _train(compressed, opt_c, ddp_c)
    for name, p in compressed.named_parameters():
        assert _in_bucket(ddp_c, p.grad), name + ".grad left the bucket"
