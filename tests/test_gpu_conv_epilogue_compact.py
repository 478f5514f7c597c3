"""The compact pooled conv epilogue (``conv_bias_relu(..., pool=True,
keep_y=False)``: csrc/epilogue_kernels.hip's code-writing forward and
code-reading backward) against its two references on the same GPU, bit for
bit: the ``keep_y=True`` kernel path (p, dx and the bias gradient) and
torch's own chain add_, relu_, max_pool2d and their backward (p and dx).
GPU-only."""

import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

NAN = float("nan")
# 2x2 windows as (h0w0, h0w1, h1w0, h1w1), values of x + b
PATTERNS = (
    [[-1.0, -2.0, -0.5, -3.0],          # all negative
     [2.0, 2.0, 0.5, 0.5],              # exact ties of the maximum
     [0.5, 2.0, 0.5, 2.0],
     [0.0, 0.0, -1.0, -0.5],            # ties at zero
     [-1.0, 0.0, -0.5, 0.0]]
    # a NaN at each position, then two in one window
    + [[NAN if k == j else 0.25 * (k + 1) for k in range(4)]
       for j in range(4)]
    + [[NAN, 1.0, NAN, 0.5], [1.0, NAN, 3.0, NAN],
       [-0.0, -1.0, -2.0, -0.5],        # the maximum is a negative zero
       [3.0, 1.0, 0.5, 2.0]]            # a live winner; its g is -0.0
)
LIVE = len(PATTERNS) - 1
# a prepared window in every third (pooled row, even channel) slot
EVERY = 3

# name: (dtype, N, H, W, C). bf16 and f16 lanes hold 8 channels, f32 lanes 4;
# a block is C/8 (C/4) lanes by 256 // lanes windows.
CASES = {
    "one_window_bf16": (torch.bfloat16, 1, 2, 2, 8),
    "one_window_f32": (torch.float32, 1, 2, 2, 4),
    # 3 lanes per window, 85 windows per block and one to do: idle lanes
    "three_vectors_bf16": (torch.bfloat16, 1, 2, 2, 24),
    "c512_bf16": (torch.bfloat16, 2, 4, 4, 512),
    # windows straddle rows and images
    "n3_4x6_bf16": (torch.bfloat16, 3, 4, 6, 64),
    # C = 512: 4 windows per block and the reducing grid is capped at 256
    # blocks, 1024 windows a round; 2 * 17 * 32 = 1088 windows need a second
    # round from 16 of the blocks
    "second_round_bf16": (torch.bfloat16, 2, 34, 64, 512),
    # 2 * 65 * 64 = 8320 windows: more than the forward's 2048 blocks cover
    # in one round, too
    "forward_second_round_bf16": (torch.bfloat16, 2, 130, 128, 512),
    # 120 windows of 3 lanes on 85 per block: two blocks, one partly filled
    "three_vectors_f32": (torch.float32, 2, 12, 20, 12),
    "c64_f16": (torch.float16, 2, 6, 10, 64),
}


def _slots(name):
    _, n, h, w, c = CASES[name]
    return n * (h // 2) * (w // 2) * (c // 2)


# cases in which every prepared pattern occurs, four times or more
ROOMY = sorted(k for k in CASES if _slots(k) >= 4 * EVERY * len(PATTERNS))


def _bits(t):
    return t.contiguous().view(
        torch.int32 if t.dtype == torch.float32 else torch.int16)


def _bit_equal(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _make_inputs(name, device="cuda"):
    """x, b and the pooled gradient g of a case, seeded. Even channels hold
    quarter-integers (x + b is exact in all three dtypes, ties abound) with
    the prepared windows among them, odd channels arbitrary values, so that
    x + b has to round."""
    dtype, n, h, w, c = CASES[name]
    ho, wo = h // 2, w // 2
    orows = n * ho * wo
    gen = torch.Generator(device=device).manual_seed(
        sum(ord(ch) for ch in name) * 7919 + c)
    f64 = dict(dtype=torch.float64, device=device)

    def quarters(lo, hi, shape):
        return torch.randint(lo, hi + 1, shape, generator=gen,
                             device=device).double() * 0.25

    b = quarters(-8, 8, (c,))
    rnd_b = torch.randn(c, generator=gen, **f64)
    b[1::2] = rnd_b[1::2]
    pre = quarters(-12, 12, (orows, c, 4))      # x + b, window by window
    g = torch.randn(orows, c, generator=gen, **f64)
    g.view(-1)[::7] = -0.0
    g.view(-1)[3::11] = 0.0
    ce = c // 2
    s = torch.arange(0, orows * ce, EVERY, device=device)
    pid = (s // EVERY) % len(PATTERNS)
    o, ch = s // ce, 2 * (s % ce)
    pre[o, ch] = torch.tensor(PATTERNS, **f64)[pid]
    g[o[pid == LIVE], ch[pid == LIVE]] = -0.0

    def full(win):  # [orows, C, 4] windows -> (N, C, H, W)
        return win.view(n, ho, wo, c, 2, 2).permute(0, 3, 1, 4, 2, 5) \
            .reshape(n, c, h, w)

    x = full(pre) - b.view(1, -1, 1, 1)
    rnd = torch.randn(n, c, h, w, generator=gen, **f64) * 2
    x[:, 1::2] = rnd[:, 1::2]
    # -0.0 + -0.0 is the only sum that is -0.0: channels 0, 8, ... get a
    # -0.0 bias and x = x + b itself, with more negative zeros sprinkled in
    b[0::8] = -0.0
    x[:, 0::8] = full(pre)[:, 0::8]
    sprinkle = torch.rand(n, h, w, generator=gen, device=device) < 0.125
    x[:, 0][sprinkle] = -0.0
    cl = dict(memory_format=torch.channels_last)
    g = g.view(n, ho, wo, c).permute(0, 3, 1, 2)
    return (x.to(dtype).contiguous(**cl), b.to(dtype),
            g.to(dtype).contiguous(**cl))


def _pattern_census(x, b, g):
    """Which of the prepared situations the inputs of a case hold, from the
    values themselves and not from how they were planted."""
    n, c, h, w = x.shape
    pre = x.clone().add_(b.view(1, -1, 1, 1))   # rounded to dtype, as y is
    win = pre.float().view(n, c, h // 2, 2, w // 2, 2) \
        .permute(0, 2, 4, 1, 3, 5).reshape(-1, 4)
    gw = g.permute(0, 2, 3, 1).reshape(-1)
    nans = torch.isnan(win)
    top = win.max(1).values                     # NaN where the window has one
    ties = (win == top.unsqueeze(1)).sum(1) >= 2
    live = torch.relu(pre)
    live = F.max_pool2d(live, 2, 2).permute(0, 2, 3, 1).reshape(-1) > 0
    census = {
        "all negative": (win < 0).all(1).any(),
        "positive tie": (ties & (top > 0)).any(),
        "tie at zero": (ties & (top == 0)).any(),
        "two NaNs": (nans.sum(1) == 2).any(),
        "-0.0 gradient at a live winner":
            ((gw == 0) & torch.signbit(gw) & live).any(),
        "negative-zero pre-activation":
            ((pre == 0) & torch.signbit(pre)).any(),
    }
    for k in range(4):
        census["NaN at %d" % k] = (nans[:, k] & (nans.sum(1) == 1)).any()
    return {k: bool(v) for k, v in census.items()}


def _torch_chain(x, b, g):
    xl = x.clone().requires_grad_()
    bl = b.clone().requires_grad_()
    y = xl.clone()
    y.add_(bl.view(1, -1, 1, 1))
    y = torch.relu_(y)
    p = F.max_pool2d(y, 2, 2)
    p.backward(g)
    return p.detach(), xl.grad, bl.grad


def _fused(x, b, g, keep_y):
    """p, dx, db and the tensor the epilogue was handed, after the call"""
    from bagua_amd.ops import conv_epilogue

    assert conv_epilogue.kernels_apply(x, b, True)
    xl = x.clone().requires_grad_()
    bl = b.clone().requires_grad_()
    conv_out = xl.clone()
    p = conv_epilogue.conv_bias_relu(conv_out, bl, True, keep_y=keep_y)
    p.backward(g)
    return p.detach(), xl.grad, bl.grad, conv_out.detach()


@functools.lru_cache(maxsize=None)
def _results(name):
    """Inputs, torch's chain, the keep_y=True path and two compact runs of
    one case, computed once and shared (read-only) by the tests below."""
    x, b, g = _make_inputs(name)
    r = dict(x=x, b=b, g=g, ref=_torch_chain(x, b, g),
             kept=_fused(x, b, g, True), got=_fused(x, b, g, False),
             again=_fused(x, b, g, False))
    torch.cuda.synchronize()
    return r


@requires_gpu
@pytest.mark.parametrize("name", ROOMY)
def test_inputs_hold_the_patterns(name):
    r = _results(name)
    census = _pattern_census(r["x"], r["b"], r["g"])
    assert all(census.values()), census


def test_roomy_cases():
    # all but the three single-window ones
    assert set(CASES) - set(ROOMY) == {
        "one_window_bf16", "one_window_f32", "three_vectors_bf16"}


@requires_gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_bitwise_against_kept_y_path(name):
    r = _results(name)
    for what, a, ref in zip(("p", "dx", "db"), r["got"], r["kept"]):
        assert a.dtype == CASES[name][0]
        assert _bit_equal(a, ref), what
    assert r["got"][0].is_contiguous(memory_format=torch.channels_last)
    assert r["got"][1].is_contiguous(memory_format=torch.channels_last)


@requires_gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_bitwise_against_torch_chain(name):
    r = _results(name)
    assert _bit_equal(r["got"][0], r["ref"][0]), "p"
    assert _bit_equal(r["got"][1], r["ref"][1]), "dx"


@requires_gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_two_runs_identical(name):
    r = _results(name)
    for what, a, ref in zip(("p", "dx", "db"), r["got"], r["again"]):
        assert _bit_equal(a, ref), what


@requires_gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_conv_output_is_left_alone(name):
    r = _results(name)
    assert _bit_equal(r["got"][3], r["x"])
    if name in ROOMY:  # whereas the keep_y=True path has written y there
        assert not _bit_equal(r["kept"][3], r["x"])


@requires_gpu
def test_torch_bias_grad_switch_is_bitwise():
    from bagua_amd.ops import conv_epilogue

    r = _results("n3_4x6_bf16")
    xl = r["x"].clone().requires_grad_()
    bl = r["b"].clone().requires_grad_()
    p = conv_epilogue.conv_bias_relu(xl.clone(), bl, True, True,
                                     keep_y=False)
    p.backward(r["g"])
    assert _bit_equal(xl.grad, r["ref"][1])
    assert _bit_equal(bl.grad, r["ref"][2])


@requires_gpu
def test_graph_capture_and_replay():
    from bagua_amd.ops import conv_epilogue

    x, b, g = _make_inputs("n3_4x6_bf16")
    x = x[:2, :8, :4, :4].contiguous(memory_format=torch.channels_last)
    g = g[:2, :8, :2, :2].contiguous(memory_format=torch.channels_last)
    b = b[:8].contiguous()
    assert x.shape == (2, 8, 4, 4)
    xs = torch.zeros_like(x).requires_grad_()
    bs = torch.zeros_like(b).requires_grad_()
    gs = torch.zeros_like(g)

    def run():
        out = conv_epilogue.conv_bias_relu(xs * 1, bs, True, keep_y=False)
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
    # three replays on two sets of inputs, each against the eager results
    for xi, gi in ((x, g), (x.flip(0), -g), (x, g)):
        xi = xi.contiguous(memory_format=torch.channels_last)
        with torch.no_grad():
            xs.copy_(xi)
            bs.copy_(b)
            gs.copy_(gi)
        graph.replay()
        torch.cuda.synchronize()
        p_ref, dx_ref, _ = _torch_chain(xi, b, gi)
        eager = _fused(xi, b, gi, False)
        assert _bit_equal(outs[0], p_ref)
        assert _bit_equal(outs[1], dx_ref)
        assert _bit_equal(outs[2], eager[2])


@requires_gpu
def test_vgg_prefix_same_bits_with_and_without(monkeypatch):
    """VGG16's features through the second pool, with the pooled stages
    compact (the model's default) and keeping y."""
    from bagua_amd.models.vgg import VGG
    from bagua_amd.ops import conv_epilogue

    torch.manual_seed(5)
    model = VGG([64, 64, "M", 128, 128, "M"], num_classes=10)
    model = model.cuda().to(torch.bfloat16).to(
        memory_format=torch.channels_last)
    x = torch.randn(2, 3, 16, 16, device="cuda", dtype=torch.bfloat16) \
        .contiguous(memory_format=torch.channels_last)
    calls = []
    kept, compact_entry = (conv_epilogue.conv_bias_relu,
                           conv_epilogue.conv_bias_relu_pool)

    def spy_kept(conv_out, bias, pool=False, torch_bias_grad=False):
        calls.append(("keeps y", pool,
                      conv_epilogue.kernels_apply(conv_out, bias, pool)))
        return kept(conv_out, bias, pool, torch_bias_grad)

    def spy_compact(conv_out, bias, torch_bias_grad=False):
        calls.append(("compact", True,
                      conv_epilogue.kernels_apply(conv_out, bias, True)))
        return compact_entry(conv_out, bias, torch_bias_grad)

    monkeypatch.setattr(conv_epilogue, "conv_bias_relu", spy_kept)
    monkeypatch.setattr(conv_epilogue, "conv_bias_relu_pool", spy_compact)

    def run(compact):
        monkeypatch.setattr(VGG, "compact_pool_epilogue", compact)
        model.zero_grad(set_to_none=True)
        out = model._features(x)
        out.float().square().sum().backward()
        return out.detach(), [p.grad.clone() for p in model.parameters()
                              if p.grad is not None]

    assert VGG.compact_pool_epilogue is True
    out_c, grads_c = run(True)
    # the first stage is ops/first_conv's; convolutions 2 and 4 are pooled
    assert calls == [("compact", True, True), ("keeps y", False, True),
                     ("compact", True, True)]
    del calls[:]
    out_k, grads_k = run(False)
    assert calls == [("keeps y", True, True), ("keeps y", False, True),
                     ("keeps y", True, True)]
    assert out_c.shape == (2, 128, 4, 4)
    assert _bit_equal(out_c, out_k)
    assert len(grads_c) == len(grads_k) == 8  # 4 weights, 4 biases
    for a, k in zip(grads_c, grads_k):
        assert _bit_equal(a, k)
