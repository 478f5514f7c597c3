"""gfx950 conv-epilogue kernels (csrc/epilogue_kernels.hip) against torch's
own chain on the same GPU: channels-last input, in-place bias add_, relu_,
max_pool2d and their autograd backward. y, p and dx must match bit for bit;
the bias gradient is held to the error bound of an f32 sum. GPU-only."""

import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

NAN = float("nan")
# 2x2 windows as (h0w0, h0w1, h1w0, h1w1), values of x + b
PATTERNS = (
    # an exact positive tie that starts at each of the four positions
    [[2.0 if k in (j, (j + 1) % 4) else 0.5 for k in range(4)]
     for j in range(4)]
    + [[1.25, 1.25, 1.25, 1.25],
       [0.0, 0.0, 0.0, 0.0],            # all zero
       [-1.0, -2.0, -0.5, -3.0],        # all negative
       [-1.0, 0.0, -0.5, 0.0]]
    # a NaN at each position, then two in one window
    + [[NAN if k == j else 0.25 * (k + 1) for k in range(4)]
       for j in range(4)]
    + [[NAN, 1.0, NAN, 0.5], [1.0, NAN, 3.0, NAN], [NAN, NAN, NAN, NAN]]
)

# name: (dtype, N, H, W, C)
CASES = {
    "one_vector_f32": (torch.float32, 1, 2, 2, 4),
    "one_vector_f16": (torch.float16, 1, 2, 2, 8),
    "one_vector_bf16": (torch.bfloat16, 1, 2, 2, 8),
    # 3 lanes per row, 85 row-lanes per block: 4 rows leave most idle
    "three_vectors_few_rows": (torch.bfloat16, 1, 2, 2, 24),
    # 120 rows on 85 row-lanes: two blocks, the second partly filled
    "three_vectors_f32": (torch.float32, 2, 6, 10, 12),
    "c64_f32": (torch.float32, 2, 6, 10, 64),
    "c64_f16": (torch.float16, 2, 6, 10, 64),
    "c64_bf16": (torch.bfloat16, 2, 6, 10, 64),
    # 32768 rows of 64 channels (4 MB): the reducing grids are capped and
    # each of their blocks iterates more than once
    "many_rows_bf16": (torch.bfloat16, 2, 128, 128, 64),
    "many_rows_tail_f32": (torch.float32, 3, 94, 62, 32),
    "c512_bf16": (torch.bfloat16, 2, 14, 14, 512),
    # 33280 rows on 4 row-lanes: the smallest size at which the forward
    # grid (2048 blocks) too is capped and its four-rows-at-a-time loop
    # runs, followed by its tail; the backward loops run 8 times
    "unrolled_loops_bf16": (torch.bfloat16, 2, 130, 128, 512),
}


def _bits(t):
    return t.contiguous().view(
        torch.int32 if t.dtype == torch.float32 else torch.int16)


def _bit_equal(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _make_inputs(name):
    dtype, n, h, w, c = CASES[name]
    gen = torch.Generator().manual_seed(
        sum(ord(ch) for ch in name) * 7919 + c)
    # quarter-integers: x + b is exact in all three dtypes, ties abound
    b = torch.randint(-8, 9, (c,), generator=gen).double() * 0.25
    t = torch.randint(-12, 13, (n, c, h, w), generator=gen).double() * 0.25
    # every other channel: arbitrary values, so that x + b has to round
    rnd = torch.randn(n, c, h, w, generator=gen, dtype=torch.float64) * 2
    t[:, 1::2] = rnd[:, 1::2]
    # every other window of the even channels takes a prepared pattern
    win = t.view(n, c, h // 2, 2, w // 2, 2).permute(0, 2, 4, 1, 3, 5)
    win = win.reshape(-1, 4)
    pat = torch.tensor(PATTERNS, dtype=torch.float64)
    ids = torch.arange(win.shape[0])
    chan = ids % c
    take = (chan % 2 == 0) & ((ids // c) % 2 == 0)
    win[take] = pat[(ids[take] // 2) % len(PATTERNS)]
    t = win.view(n, h // 2, w // 2, c, 2, 2).permute(0, 3, 1, 4, 2, 5)
    t = t.reshape(n, c, h, w)
    x = t - b.view(1, -1, 1, 1)
    x[:, 1::2] = rnd[:, 1::2]
    # -0.0: with a -0.0 bias the sum is -0.0 too
    b[0] = -0.0
    zero_rows = torch.rand(n, h, w, generator=gen) < 0.25
    x[:, 0][zero_rows] = -0.0
    x = x.to(dtype).contiguous(memory_format=torch.channels_last)
    g_full = torch.randn(n, c, h, w, generator=gen)
    g_pool = torch.randn(n, c, h // 2, w // 2, generator=gen)
    for g in (g_full, g_pool):
        flat = g.view(-1)
        flat[::7] = -0.0
        flat[3::11] = 0.0
    to_cl = dict(memory_format=torch.channels_last)
    return (x.cuda(), b.to(dtype).cuda(),
            g_full.to(dtype).contiguous(**to_cl).cuda(),
            g_pool.to(dtype).contiguous(**to_cl).cuda())


def _torch_chain(x, b, g, pool):
    xl = x.clone().requires_grad_()
    bl = b.clone().requires_grad_()
    y = xl.clone()
    y.add_(bl.view(1, -1, 1, 1))
    y = torch.relu_(y)
    out = F.max_pool2d(y, 2, 2) if pool else y
    out.backward(g)
    return y.detach(), out.detach(), xl.grad, bl.grad


def _fused(x, b, g, pool, torch_bias_grad=False):
    from bagua_amd.ops import conv_epilogue

    assert conv_epilogue.kernels_apply(x, b, pool)
    xl = x.clone().requires_grad_()
    bl = b.clone().requires_grad_()
    y = xl.clone()
    out = conv_epilogue.conv_bias_relu(y, bl, pool, torch_bias_grad)
    out.backward(g)
    return y.detach(), out.detach(), xl.grad, bl.grad


@functools.lru_cache(maxsize=None)
def _results(name, pool):
    """Inputs, torch's chain and two fused runs of one case, computed once
    and shared (read-only) by the tests below."""
    x, b, g_full, g_pool = _make_inputs(name)
    g = g_pool if pool else g_full
    ref = _torch_chain(x, b, g, pool)
    got = _fused(x, b, g, pool)
    again = _fused(x, b, g, pool)
    torch.cuda.synchronize()
    return dict(x=x, b=b, g=g, ref=ref, got=got, again=again)


def _half_ulp(v, dtype):
    """Half a unit in the last place of ``dtype`` at the float64 values
    ``v``: one correct rounding of v is at most this far from it."""
    fi = torch.finfo(dtype)
    digits = round(-math.log2(fi.eps)) + 1          # with the hidden bit
    e_min = round(math.log2(fi.smallest_normal))
    _, e = torch.frexp(v)                           # |v| in [2^(e-1), 2^e)
    e = torch.where(v == 0, torch.full_like(e, e_min),
                    (e - 1).clamp(min=e_min))
    return torch.ldexp(torch.ones_like(v), e - digits)


def _bias_grad_bound(dx, dtype):
    rows = dx.shape[0] * dx.shape[2] * dx.shape[3]
    d64 = dx.double()
    s64 = d64.sum((0, 2, 3))
    bound = 2.0 ** -24 * rows * d64.abs().sum((0, 2, 3)) \
        + _half_ulp(s64, dtype)
    return s64, bound


@requires_gpu
@pytest.mark.parametrize("pool", [False, True])
@pytest.mark.parametrize("name", sorted(CASES))
def test_forward_and_dx_bitwise(name, pool):
    r = _results(name, pool)
    y_ref, out_ref, dx_ref, _ = r["ref"]
    y, out, dx, _ = r["got"]
    if y_ref.numel() >= 7680:  # room for every prepared pattern
        assert torch.isnan(y_ref).any() and (y_ref == 0).any()
        assert torch.signbit(r["x"][:, 0]).any()
    assert _bit_equal(y, y_ref), "y"
    assert _bit_equal(out, out_ref), "p" if pool else "y (returned)"
    assert out.is_contiguous(memory_format=torch.channels_last)
    assert _bit_equal(dx, dx_ref), "dx"
    assert dx.is_contiguous(memory_format=torch.channels_last)


@requires_gpu
@pytest.mark.parametrize("pool", [False, True])
@pytest.mark.parametrize("name", sorted(CASES))
def test_bias_grad_within_f32_sum_bound(name, pool):
    r = _results(name, pool)
    dtype = CASES[name][0]
    dx_ref = r["ref"][2]
    db_ref = dx_ref.sum((0, 2, 3))  # torch's own reduction of the same dx
    db = r["got"][3]
    assert db.dtype == dtype and db.shape == r["b"].shape
    s64, bound = _bias_grad_bound(dx_ref, dtype)
    assert torch.isfinite(s64).all()
    err = (db.double() - s64).abs()
    err_ref = (db_ref.double() - s64).abs()
    print("%s pool=%s: fused max err/bound %.3g, torch %.3g"
          % (name, pool, (err / bound).max().item(),
             (err_ref / bound).max().item()))
    # the bound is one the reference meets on these inputs
    assert (err_ref <= bound).all()
    assert (err <= bound).all()


@requires_gpu
@pytest.mark.parametrize("pool", [False, True])
@pytest.mark.parametrize("name", sorted(CASES))
def test_bias_grad_deterministic(name, pool):
    r = _results(name, pool)
    assert _bit_equal(r["got"][3], r["again"][3])
    assert _bit_equal(r["got"][2], r["again"][2])


@requires_gpu
@pytest.mark.parametrize("pool", [False, True])
@pytest.mark.parametrize("name", ["three_vectors_f32", "c64_bf16"])
def test_torch_bias_grad_switch_is_bitwise(name, pool):
    r = _results(name, pool)
    got = _fused(r["x"], r["b"], r["g"], pool, torch_bias_grad=True)
    assert _bit_equal(got[2], r["ref"][2])
    assert _bit_equal(got[3], r["ref"][2].sum((0, 2, 3)))
    assert _bit_equal(got[3], r["ref"][3])


@requires_gpu
def test_declined_inputs_take_torch_path():
    from bagua_amd.ops import conv_epilogue

    gen = torch.Generator().manual_seed(11)
    for shape, pool in (((2, 8, 5, 6), True),     # odd H
                        ((2, 3, 4, 4), False)):   # C = 3
        x = torch.randn(shape, generator=gen).to(torch.bfloat16).cuda()
        x = x.contiguous(memory_format=torch.channels_last)
        b = torch.randn(shape[1], generator=gen).to(torch.bfloat16).cuda()
        assert not conv_epilogue.kernels_apply(x, b, pool)
        got = conv_epilogue.conv_bias_relu(x.clone(), b, False)
        assert _bit_equal(got, F.relu(x + b.view(1, -1, 1, 1)))
    x = torch.randn(2, 8, 4, 4, generator=gen).to(torch.bfloat16).cuda()
    b = torch.zeros(8, dtype=torch.bfloat16, device="cuda")
    assert not conv_epilogue.kernels_apply(x, b, False)  # NCHW
    cl = x.contiguous(memory_format=torch.channels_last)
    assert conv_epilogue.kernels_apply(cl, b, True)
    assert not conv_epilogue.kernels_apply(cl, b.float(), True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert not conv_epilogue.kernels_apply(cl, b, True)


@requires_gpu
def test_graph_capture_and_replay():
    from bagua_amd.ops import conv_epilogue

    x, b, _, g = _make_inputs("c64_bf16")
    x, g = x[:, :8, :4, :4], g[:, :8, :2, :2]
    x = x.contiguous(memory_format=torch.channels_last)
    g = g.contiguous(memory_format=torch.channels_last)
    b = b[:8].contiguous()
    assert x.shape == (2, 8, 4, 4)
    xs = torch.zeros_like(x).requires_grad_()
    bs = torch.zeros_like(b).requires_grad_()
    gs = torch.zeros_like(g)

    def run():
        out = conv_epilogue.conv_bias_relu(xs * 1, bs, True)
        return (out,) + torch.autograd.grad(out, (xs, bs), gs)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run()
    with torch.no_grad():
        xs.copy_(x)
        bs.copy_(b)
        gs.copy_(g)
    graph.replay()
    torch.cuda.synchronize()
    _, p_ref, dx_ref, _ = _torch_chain(x, b, g, True)
    eager = _fused(x, b, g, True)
    assert _bit_equal(outs[0], p_ref)
    assert _bit_equal(outs[1], dx_ref)
    assert _bit_equal(outs[2], eager[3])
