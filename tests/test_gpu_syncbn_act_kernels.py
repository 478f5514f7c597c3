"""``SyncBatchNorm(x, residual=z, relu=True)`` on its gfx950 kernels against
float64 with the declined torch path as the yardstick, the sign mask of the
rows layout, memory format and determinism. World size 1. GPU-only."""

import functools
import math
import os
import socket

import pytest
import torch

from bagua_amd.ops import batchnorm as bn_ops

pytestmark = pytest.mark.gpu
requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
EPS = 1e-5
# name: (dtype, shape, channels_last, affine, running); affine and running
# are None, "f32" or "same" (the input's dtype)
CASES = {
    # rows: 8 mask bits; 4 bits, partly filled second block; two channel
    # tiles (mask index through blockIdx.y); grid-stride with a tail; 2-d
    "rows_one_vector": (BF16, (1, 8, 2, 1), True, "f32", "f32"),
    "rows_second_block": (F32, (3, 12, 4, 10), True, None, None),
    "rows_two_tiles": (F32, (2, 2048, 2, 2), True, "f32", None),
    "rows_capped_grid": (F32, (1, 1024, 3,
                               (2 * bn_ops.ROWS_APPLY_MAX_GRID + 5) // 3),
                         True, "f32", "f32"),
    "rows_2d": (BF16, (6, 16), False, "same", "same"),
    # planes: misaligned element loads; vector loads; blocks with a tail
    "planes_scalar": (BF16, (2, 3, 5, 5), False, "f32", "f32"),
    "planes_vector": (F16, (3, 2, 8, 8), False, "same", None),
    "planes_splits": (F32, (3, 2, 94, 62), False, None, "f32"),
}
RUNS = [(n, m) for n in sorted(CASES) for m in ("relu", "add_relu")]


@pytest.fixture(scope="module", autouse=True)
def _world_of_one():
    if not torch.cuda.is_available():
        return
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    for key, value in (("WORLD_SIZE", "1"), ("RANK", "0"),
                       ("LOCAL_RANK", "0"), ("MASTER_ADDR", "127.0.0.1"),
                       ("MASTER_PORT", str(port))):
        os.environ.setdefault(key, value)
    import bagua_amd

    torch.cuda.set_device(0)
    bagua_amd.init_process_group()


def _make(name):
    """Seeded as in test_gpu_syncbn_kernels.py (about half of a channel's
    pre-activations are positive), plus a residual z ~ randn."""
    dtype, shape, cl, affine, running = CASES[name]
    gen = torch.Generator().manual_seed(sum(map(ord, name)) * 7919)
    c = shape[1]
    view = (1, c) + (1,) * (len(shape) - 2)
    std = torch.rand(c, generator=gen) + 0.5
    mean = (torch.rand(c, generator=gen) * 4 - 2) * std
    x = torch.randn(shape, generator=gen) * std.view(view) + mean.view(view)
    g, z = torch.randn(shape, generator=gen), torch.randn(shape, generator=gen)
    fmt = torch.channels_last if cl else torch.contiguous_format
    x, g, z = (t.to(dtype).cuda().contiguous(memory_format=fmt)
               for t in (x, g, z))
    kind = {None: None, "f32": F32, "same": dtype}
    params = {}
    for key, base, dt in (("weight", 1.0, kind[affine]),
                          ("bias", 0.0, kind[affine]),
                          ("running_mean", 0.0, kind[running]),
                          ("running_var", 1.0, kind[running])):
        noise = torch.rand(c, generator=gen) - 0.5
        params[key] = None if dt is None else (base + noise).to(dt).cuda()
    return x, g, z, params


def _step(name, mode, module_cls, masks=None):
    """One step of relu(bn(x) [+ z]): SyncBatchNorm's fused call, or with
    ``masks`` float64 modules and, per y in it, gradients of g * (y > 0)."""
    x, g, z, params = _make(name)
    ref = masks is not None
    bn = module_cls(x.shape[1], eps=EPS, affine=params["weight"] is not None,
                    track_running_stats=params["running_mean"] is not None)
    bn = bn.cuda()
    for key, value in params.items():
        if value is not None:
            getattr(bn, key).data = value.double() if ref else value
    if ref:
        x, g, z = x.double(), g.double(), z.double()
    leaves = dict(dx=x.requires_grad_())
    if mode == "add_relu":
        leaves["dz"] = z.requires_grad_()
    if bn.affine:
        leaves.update(grad_weight=bn.weight, grad_bias=bn.bias)
    if ref:
        pre = bn(x) + z if mode == "add_relu" else bn(x)
        res = [dict(zip(leaves, torch.autograd.grad(
            pre, list(leaves.values()), g * (y > 0), retain_graph=True)))
            for y in masks]
        res[0]["y"] = torch.relu(pre).detach()
    else:
        out = bn(x, residual=leaves.get("dz"), relu=True)
        res = [dict(zip(leaves, torch.autograd.grad(
            out, list(leaves.values()), g)), y=out.detach())]
    if bn.track_running_stats:
        res[0].update(running_mean=bn.running_mean,
                      running_var=bn.running_var)
    return res


@functools.lru_cache(maxsize=None)
def _runs(name, mode):
    """Kernels (twice), declined torch path, float64; shared, read-only."""
    from bagua_amd.contrib import SyncBatchNorm

    x, _, _, p = _make(name)
    assert bn_ops.kernels_apply(x, p["weight"], p["bias"], p["running_mean"],
                                p["running_var"], 0.1)
    got, = _step(name, mode, SyncBatchNorm)
    again, = _step(name, mode, SyncBatchNorm)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(bn_ops, "kernels_apply", lambda *a, **k: False)
        chain, = _step(name, mode, SyncBatchNorm)
    ref_cls = torch.nn.BatchNorm2d if x.dim() == 4 else torch.nn.BatchNorm1d
    ref_got, ref_chain = _step(name, mode, ref_cls, (got["y"], chain["y"]))
    torch.cuda.synchronize()
    return dict(x=x, got=got, again=again, chain=chain, ref_got=ref_got,
                ref_chain=ref_chain)


@requires_gpu
@pytest.mark.parametrize("name,mode", RUNS)
def test_fused_module_against_float64(name, mode):
    """The rule of test_gpu_syncbn_kernels.py: at most twice the declined
    torch path's error plus half an ulp at the reference's largest
    magnitude. Each path's gradients are judged under its own mask, so a
    sign that differs within an ulp of zero is not counted as a whole dy."""
    r = _runs(name, mode)
    assert r["got"].keys() == r["chain"].keys() == r["ref_got"].keys()
    for key, ref in r["ref_got"].items():
        got, chain = r["got"][key], r["chain"][key]
        ref_chain = r["ref_chain"].get(key, ref)  # forward: one reference
        assert got.shape == ref.shape and got.dtype == chain.dtype
        assert torch.isfinite(ref).all()
        fi = torch.finfo(got.dtype)
        top = max(ref.abs().max().item(), fi.tiny)
        half_ulp = 0.5 * fi.eps * 2.0 ** math.floor(math.log2(top))
        err = (got.double() - ref).abs().max().item()
        err_base = (chain.double() - ref_chain).abs().max().item()
        print("%s %s %s: kernels %.3g, yardstick %.3g, half ulp %.3g, ratio "
              "%.3g" % (name, mode, key, err, err_base, half_ulp,
                        err / err_base if err_base else float("inf")))
        assert err <= 2 * err_base + half_ulp, key


@requires_gpu
@pytest.mark.parametrize("name,mode", RUNS)
def test_saved_sign_mask(name, mode):
    """Rows: a byte per 16-byte vector of the stored y, bit k for element k.
    Planes: y itself."""
    x, _, z, p = _make(name)
    y, _, act = bn_ops.apply_act(
        x, bn_ops.stats(x), p["weight"], p["bias"], p["running_mean"],
        p["running_var"], 0.1, EPS, z if mode == "add_relu" else None)
    assert torch.equal(y, _runs(name, mode)["got"]["y"])
    if name.startswith("planes"):
        assert act is y
        return
    v = 16 // x.element_size()
    rows = y.permute(0, 2, 3, 1) if y.dim() == 4 else y
    bits = (rows.reshape(-1, x.shape[1] // v, v) > 0).int()
    want = (bits << torch.arange(v, device="cuda")).sum(-1).to(torch.uint8)
    assert 0 < bits.sum().item() < bits.numel()
    assert act.dtype == torch.uint8 and torch.equal(act, want)


@requires_gpu
@pytest.mark.parametrize("name,mode", RUNS)
def test_fused_memory_format_and_determinism(name, mode):
    r = _runs(name, mode)
    for key in {"y", "dx", "dz"} & r["got"].keys():
        assert r["got"][key].stride() == r["x"].stride(), key
    for key, t in r["got"].items():
        assert torch.equal(t.contiguous().view(torch.uint8),
                           r["again"][key].contiguous().view(torch.uint8)), key
