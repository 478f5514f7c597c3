"""gfx950 batch-norm kernels (csrc/batchnorm_kernels.hip) behind
``contrib.SyncBatchNorm``: their sums against float64 with the error bound
of an f32 sum, the module against ``nn.BatchNorm`` in float64 with the torch
chain it replaces as the yardstick, the two-rank protocol without
communication, memory format, determinism and the declined inputs.
World size 1. GPU-only."""

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
V = {F32: 4, F16: 8, BF16: 8}  # elements of a 16-byte vector
EPS = 1e-5

# name: (dtype, shape, channels_last, affine, running); affine and running
# are None, "f32" or "same" (the input's dtype)
CASES = {
    # rows layout [N*H*W, C]
    # one 16-byte vector of channels, two rows
    "rows_one_vector": (BF16, (1, V[BF16], 2, 1), True, "f32", "f32"),
    # 3 lanes along C, 85 row-lanes of which 4 have a row
    "rows_three_vectors_few_rows": (F16, (1, 3 * V[F16], 2, 2), True, "same",
                                    "same"),
    # 120 rows on 85 row-lanes: two blocks, the second partly filled
    "rows_second_block": (F32, (3, 3 * V[F32], 4, 10), True, None, None),
    # 512 channel vectors: two channel tiles of 256 lanes, one row-lane
    "rows_two_tiles": (F32, (2, 2048, 2, 2), True, "f32", None),
    # 256 lanes, one row-lane: 2 * 2048 + 5 rows is the fewest at which the
    # capped apply grids make every block loop twice and leave a tail (the
    # reducing grids, capped at 128 blocks, loop 32 times)
    "rows_capped_grid": (F32, (1, 256 * V[F32], 3,
                               (2 * bn_ops.ROWS_APPLY_MAX_GRID + 5) // 3),
                         True, "f32", "f32"),
    # 2-d input: inner size 1
    "rows_2d": (BF16, (6, 2 * V[BF16]), False, "f32", "f32"),
    # planes layout [N, C, S]
    # 50-byte planes: element loads, segments start misaligned
    "planes_scalar": (BF16, (2, 3, 5, 5), False, "f32", "f32"),
    "planes_vector": (F16, (3, 2, 8, 8), False, "same", None),
    "planes_3d": (F32, (4, 6, 10), False, None, "f32"),
    # 4371 vectors per channel on 5 blocks: 3 full turns and a tail
    "planes_splits": (F32, (3, 2, 94, 62), False, "f32", "f32"),
}
ROWS_HALVES, PLANES_HALVES = "rows_second_block", "planes_vector"


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
    """Seeded x ~ randn * std_c + mean_c with |mean_c| <= 2 std_c, the
    upstream gradient g, and per-channel parameters, all rounded to their
    dtypes and on the GPU in the case's memory format."""
    dtype, shape, cl, affine, running = CASES[name]
    gen = torch.Generator().manual_seed(sum(map(ord, name)) * 7919)
    c = shape[1]
    view = (1, c) + (1,) * (len(shape) - 2)
    std = torch.rand(c, generator=gen) + 0.5
    mean = (torch.rand(c, generator=gen) * 4 - 2) * std
    x = torch.randn(shape, generator=gen) * std.view(view) + mean.view(view)
    g = torch.randn(shape, generator=gen)
    fmt = torch.channels_last if cl else torch.contiguous_format
    x, g = (t.to(dtype).cuda().contiguous(memory_format=fmt) for t in (x, g))
    kind = {None: None, "f32": F32, "same": dtype}
    params = {}
    for key, base, dt in (("weight", 1.0, kind[affine]),
                          ("bias", 0.0, kind[affine]),
                          ("running_mean", 0.0, kind[running]),
                          ("running_var", 1.0, kind[running])):
        noise = torch.rand(c, generator=gen) - 0.5
        params[key] = None if dt is None else (base + noise).to(dt).cuda()
    return x, g, params


def _within(got, base, ref, what):
    """``got`` may be at most twice as far from the float64 ``ref`` as the
    yardstick ``base`` is, plus half an ulp of got's dtype at ref's largest
    magnitude: both are f32 computations with the same roundings that differ
    in summation order and FMA contraction, and either can move an element
    across one rounding boundary of the output dtype."""
    fi = torch.finfo(got.dtype)
    top = max(ref.abs().max().item(), fi.tiny)
    half_ulp = 0.5 * fi.eps * 2.0 ** math.floor(math.log2(top))
    err = (got.double() - ref).abs().max().item()
    err_base = (base.double() - ref).abs().max().item()
    print("%s: kernels %.3g, yardstick %.3g, half ulp %.3g, ratio %.3g"
          % (what, err, err_base, half_ulp,
             err / err_base if err_base else float("inf")))
    assert err <= 2 * err_base + half_ulp, what


def _module_step(name, module_cls, dtype64=False):
    """One training step of ``module_cls`` on the case; every tensor the
    tests compare, detached."""
    x, g, params = _make(name)
    c = x.shape[1]
    bn = module_cls(c, eps=EPS, affine=params["weight"] is not None,
                    track_running_stats=params["running_mean"] is not None)
    bn = bn.cuda()
    for key, value in params.items():
        if value is not None:
            getattr(bn, key).data = value.double() if dtype64 else value
    if dtype64:
        x, g = x.double(), g.double()
    x.requires_grad_()
    out = bn(x)
    # grad, not backward: dx as the function returns it, in its own strides
    grads = torch.autograd.grad(
        (out * g).sum(), [x] + ([bn.weight, bn.bias] if bn.affine else []))
    res = dict(y=out.detach(), dx=grads[0])
    if bn.affine:
        res.update(grad_weight=grads[1], grad_bias=grads[2])
    if bn.track_running_stats:
        res.update(running_mean=bn.running_mean, running_var=bn.running_var)
    return res


@functools.lru_cache(maxsize=None)
def _runs(name):
    """The case through the kernels (twice), through the torch chain they
    replace, and through nn.BatchNorm in float64; shared, read-only."""
    from bagua_amd.contrib import SyncBatchNorm

    x, _, params = _make(name)
    assert bn_ops.kernels_apply(x, params["weight"], params["bias"],
                                params["running_mean"],
                                params["running_var"], 0.1)
    got = _module_step(name, SyncBatchNorm)
    again = _module_step(name, SyncBatchNorm)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(bn_ops, "kernels_apply", lambda *a, **k: False)
        chain = _module_step(name, SyncBatchNorm)
    ref_cls = torch.nn.BatchNorm2d if x.dim() == 4 else torch.nn.BatchNorm1d
    ref = _module_step(name, ref_cls, dtype64=True)
    torch.cuda.synchronize()
    return dict(x=x, got=got, again=again, chain=chain, ref=ref)


def _channel_sums(t):
    return t.transpose(0, 1).reshape(t.shape[1], -1).sum(1)


@requires_gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_sums_within_f32_bound(name):
    """Any-order f32 summation of n terms errs by at most
    2^-24 * n * sum|t_i|; the squares add one rounding each."""
    x, g, _ = _make(name)
    c, n = x.shape[1], x.numel() // x.shape[1]
    u = 2.0 ** -24
    stats = bn_ops.stats(x)
    assert stats[2 * c].item() == n
    _, mean_invstd = bn_ops.apply(x, stats, None, None, None, None, 0.1, EPS)
    packed, _, _ = bn_ops.backward_reduce(g, x, mean_invstd)
    xmu32 = x.float() - mean_invstd[:c].view((1, c) + (1,) * (x.dim() - 2))
    x64, g64, xmu64 = x.double(), g.double(), xmu32.double()
    # (kernel result, torch's f32 sum of the same terms, float64 terms,
    #  roundings of the terms themselves)
    for what, got, torch32, t64, extra in (
            ("sum", stats[:c], _channel_sums(x.float()), x64, 0.0),
            ("sqsum", stats[c:2 * c], _channel_sums(x.float() ** 2),
             x64 * x64, u),
            ("sum_dy", packed[:c], _channel_sums(g.float()), g64, 0.0),
            ("sum_dy_xmu", packed[c:], _channel_sums(g.float() * xmu32),
             g64 * xmu64, 0.0)):
        ref = _channel_sums(t64)
        bound = (u * n + extra) * _channel_sums(t64.abs())
        err = (got.double() - ref).abs()
        err_torch = (torch32.double() - ref).abs()
        print("%s %s: kernels err/bound %.3g, torch %.3g"
              % (name, what, (err / bound).max().item(),
                 (err_torch / bound).max().item()))
        assert (err_torch <= bound).all(), what  # torch meets it too
        assert (err <= bound).all(), what


@requires_gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_module_against_float64(name):
    r = _runs(name)
    assert r["got"].keys() == r["chain"].keys() == r["ref"].keys()
    for key, ref in r["ref"].items():
        got, chain = r["got"][key], r["chain"][key]
        assert got.shape == ref.shape and got.dtype == chain.dtype
        assert torch.isfinite(ref).all()
        _within(got, chain, ref, "%s %s" % (name, key))


@requires_gpu
@pytest.mark.parametrize("name", [ROWS_HALVES, PLANES_HALVES])
def test_two_halves_make_a_batch(name):
    """The protocol of two ranks without the communication: the vectors of
    the two halves are added and each half is normalised with the sum. The
    yardstick is the same kernels on the whole batch."""
    x, g, params = _make(name)
    w, b = params["weight"], params["bias"]
    c, h = x.shape[1], x.shape[0] // 2
    assert 0 < h < x.shape[0] - h  # unequal halves
    ref = _runs(name)["ref"]

    def step(xs, gs):
        stats = sum(bn_ops.stats(xi) for xi in xs)
        fwd = [bn_ops.apply(xi, stats, w, b, None, None, 0.1, EPS)
               for xi in xs]
        packed = sum(bn_ops.backward_reduce(gi, xi, mi)[0]
                     for gi, xi, (_, mi) in zip(gs, xs, fwd))
        dx = [bn_ops.backward_apply(gi, xi, packed, stats, mi, w)
              for gi, xi, (_, mi) in zip(gs, xs, fwd)]
        return stats, torch.cat([y for y, _ in fwd]), torch.cat(dx)

    def halves(t):
        return [p.clone(memory_format=torch.preserve_format)
                for p in (t[:h], t[h:])]

    stats, y, dx = step(halves(x), halves(g))
    _, y_full, dx_full = step([x], [g])
    assert stats[2 * c].item() == x.numel() // c
    _within(y, y_full, ref["y"], name + " y")
    _within(dx, dx_full, ref["dx"], name + " dx")


@requires_gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_memory_format_and_determinism(name):
    r = _runs(name)
    x = r["x"]
    for key in ("y", "dx"):
        t = r["got"][key]
        assert t.stride() == x.stride(), key
        if CASES[name][2]:
            assert t.is_contiguous(memory_format=torch.channels_last), key
        else:
            assert t.is_contiguous(), key
    for key, t in r["got"].items():
        assert torch.equal(t.contiguous().view(torch.uint8),
                           r["again"][key].contiguous().view(torch.uint8)), key


def _misaligned(t):
    """The same values and strides, two or four bytes off alignment."""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    out = flat[1:].as_strided(t.shape, t.stride())
    return out.copy_(t)


# (what, dtype, shape, channels_last, momentum, transform of x)
DECLINED = [
    ("f64", torch.float64, (2, 4, 3, 3), False, 0.1, None),
    ("channels_last_c_not_vectors", BF16, (2, 12, 3, 3), True, 0.1, None),
    ("rows_2d_c_not_vectors", F32, (4, 5), False, 0.1, None),
    ("misaligned_base", F32, (2, 8, 3, 3), True, 0.1, _misaligned),
    ("momentum_none", F32, (2, 8, 3, 3), True, None, None),
]


@requires_gpu
@pytest.mark.parametrize("case", DECLINED, ids=[d[0] for d in DECLINED])
def test_declined_inputs_take_torch_path(case):
    from bagua_amd.contrib import SyncBatchNorm

    _, dtype, shape, cl, momentum, transform = case
    gen = torch.Generator().manual_seed(23)
    x = (torch.randn(shape, generator=gen) + 0.5).to(dtype).cuda()
    if cl:
        x = x.contiguous(memory_format=torch.channels_last)
    if transform:
        x = transform(x)
    g = torch.randn(shape, generator=gen).to(dtype).cuda()
    bn = SyncBatchNorm(shape[1], eps=EPS, momentum=momentum,
                       track_running_stats=False).cuda()
    assert not bn_ops.kernels_apply(x, bn.weight, bn.bias, None, None,
                                    momentum)
    ref_cls = torch.nn.BatchNorm2d if len(shape) == 4 \
        else torch.nn.BatchNorm1d
    ref_bn = ref_cls(shape[1], eps=EPS, track_running_stats=False)
    ref_bn = ref_bn.cuda().double()
    outs = []
    for mod, xi, gi in ((bn, x, g), (ref_bn, x.double(), g.double())):
        xi = xi.detach().requires_grad_()
        y = mod(xi)
        (y * gi).sum().backward()
        outs.append((y.detach(), xi.grad, mod.weight.grad, mod.bias.grad))
    # the torch path computes in f32 whatever the dtype
    tol = 16 * max(torch.finfo(dtype).eps, torch.finfo(F32).eps)
    for got, ref in zip(*outs):
        torch.testing.assert_close(got.double(), ref, rtol=tol,
                                   atol=tol * ref.abs().max().item())
