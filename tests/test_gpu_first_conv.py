"""gfx950 first-convolution kernels (csrc/first_conv_kernels.hip) against
float64 on the CPU: Conv2d(3, 64, 3, padding=1) + bias + ReLU forward, and
the weight and bias gradients with dx = (y <= 0) ? 0 : g formed on the fly.
GPU-only.

Forward: with s the float64 convolution and e = 32 * 2^-24 * conv(|x|, |w|)
(the worst-case error of an f32 sum of at most 32 exact products in any
order), every element must lie in [chain(s - e), chain(s + e)], where
chain(v) = relu(bf16(bf16(v) + b)) is monotone.

Backward: dx is built in float64 from the kernel's own y;
tol = P * 2^-24 * wgrad(|x|, |dx|) + 2^-8 * (|dW_exact| + first term),
P = N*H*W: an f32 sum in any order, then one bf16 rounding."""

import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

TW, TH = 32, 4  # the kernels' tile: FC_TW x FC_TH output pixels
CL = dict(memory_format=torch.channels_last)


def _lib():
    from bagua_amd.ops import native

    return native.require()


BWD_MAX_GRID = 768  # FC_BWD_MAX_GRID


def _capped_shape():
    """The backward grid is capped at 768 blocks, and block b takes the
    tiles [b * T / 768, (b + 1) * T / 768). T = 2 * 768 + 1 is the fewest
    tiles at which the grid is capped, every block loops more than once
    (two or three tiles) and the split is uneven. W = TW + 1 and H = 4k + 1
    make half of the tiles one pixel wide and the last tile row one pixel
    high (the tails), which also keeps the tensors at 3 * H * 33 pixels, the
    fewest for that many tiles with both kinds of tail: 13 MB per
    activation."""
    rows = -(-(2 * BWD_MAX_GRID + 1) // (3 * 2))  # tile rows per image, N = 3
    return (3, TH * (rows - 1) + 1, TW + 1)


SHAPES = {
    "one_pixel": (1, 1, 1),          # every tap but the centre is padding
    "tiny": (1, 2, 3),
    "small": (2, 5, 7),
    "tile_minus": (1, TH - 1, TW - 1),
    "tile_exact": (1, TH, TW),
    "tile_plus": (1, TH + 1, TW + 1),
    # several tiles, image boundaries inside one block's pixel range
    "several_tiles": (3, 17, 70),
    "capped_grid": None,             # _capped_shape()
}


def _shape(name):
    return SHAPES[name] or _capped_shape()


def _bits(t):
    return t.contiguous().view(torch.int16)


def _bit_equal(a, b):
    return a.shape == b.shape and torch.equal(_bits(a.cpu()), _bits(b.cpu()))


def _fwd(x, w, b):
    return _lib().first_conv_bias_relu(x.cuda(), w.cuda(), b.cuda())


def _bwd(g, y, x, w):
    return _lib().first_conv_bias_relu_bwd(g.cuda(), y.cuda(), x.cuda(),
                                           w.cuda())


def _wgrad64(x64, dx64):
    """float64 weight gradient (64, 3, 3, 3) of conv2d(x, w, padding=1)"""
    patches = F.unfold(x64, 3, padding=1)             # (N, 27, H*W)
    return torch.einsum("ncp,nkp->ck", dx64.flatten(2),
                        patches).view(64, 3, 3, 3)


@functools.lru_cache(maxsize=None)
def _case(name):
    """Inputs, kernel results (two backward runs) and float64 references of
    one shape, computed once and shared read-only."""
    n, h, wd = _shape(name)
    gen = torch.Generator().manual_seed(1000 + sum(map(ord, name)))
    x = torch.randn(n, 3, h, wd, generator=gen).bfloat16().contiguous(**CL)
    w = (torch.randn(64, 3, 3, 3, generator=gen) * 0.3).bfloat16()
    b = (torch.randn(64, generator=gen) * 0.5).bfloat16()
    g = torch.randn(n, 64, h, wd, generator=gen)
    flat = g.view(-1)
    flat[::7] = -0.0
    flat[3::11] = 0.0
    g = g.bfloat16().contiguous(**CL)
    y = _fwd(x, w, b)
    dw, db = _bwd(g, y, x, w)
    dw2, db2 = _bwd(g, y, x, w)
    w_cl = w.contiguous(**CL)
    y_cl = _fwd(x, w_cl, b)
    dw_cl, db_cl = _bwd(g, y, x, w_cl)
    # what the current chain gives on the same GPU
    chain = F.conv2d(x.cuda(), w.cuda(), None, 1, 1)
    chain = torch.relu_(chain.add_(b.cuda().view(1, -1, 1, 1)))
    torch.cuda.synchronize()
    x64, w64, b64 = x.double(), w.double(), b.double().view(1, -1, 1, 1)
    s = F.conv2d(x64, w64, None, 1, 1)
    e = 32 * 2.0 ** -24 * F.conv2d(x64.abs(), w64.abs(), None, 1, 1)

    def chain64(v):
        return torch.relu(v.float().bfloat16() + b.view(1, -1, 1, 1))

    y_cpu = y.cpu()
    dx64 = torch.where(y_cpu <= 0, torch.zeros_like(g), g).double()
    p = n * h * wd
    return dict(
        x=x, w=w, b=b, g=g, y=y_cpu, y_cl=y_cl.cpu(), chain=chain.cpu(),
        lo=chain64(s - e), hi=chain64(s + e),
        dw=dw, dw2=dw2, db=db, db2=db2, dw_cl=dw_cl, db_cl=db_cl,
        dw64=_wgrad64(x64, dx64),
        dw_sum=p * 2.0 ** -24 * _wgrad64(x64.abs(), dx64.abs()),
        db64=dx64.sum((0, 2, 3)),
        db_sum=p * 2.0 ** -24 * dx64.abs().sum((0, 2, 3)))


@requires_gpu
@pytest.mark.parametrize("name", list(SHAPES))
def test_forward_within_f32_sum_interval(name):
    r = _case(name)
    y = r["y"]
    n, h, wd = _shape(name)
    assert y.shape == (n, 64, h, wd) and y.dtype == torch.bfloat16
    assert y.is_contiguous(**CL)
    assert (r["lo"].float() <= r["hi"].float()).all()
    single = (r["lo"] == r["hi"]).float().mean().item()
    differ = (_bits(y) != _bits(r["chain"])).sum().item()
    print("%s: interval is one value at %.3f %% of elements; %d of %d "
          "differ from conv2d -> conv_bias_relu on this GPU"
          % (name, 100 * single, differ, y.numel()))
    yf = y.float()
    assert ((r["lo"].float() <= yf) & (yf <= r["hi"].float())).all()
    # the weight's memory format changes nothing
    assert _bit_equal(r["y_cl"], y)


@requires_gpu
@pytest.mark.parametrize("name", list(SHAPES))
def test_backward_within_f32_sum_bound(name):
    r = _case(name)
    for got, exact, first in ((r["dw"], r["dw64"], r["dw_sum"]),
                              (r["db"], r["db64"], r["db_sum"])):
        assert got.dtype == torch.bfloat16 and got.shape == exact.shape
        tol = first + 2.0 ** -8 * (exact.abs() + first)
        err = (got.cpu().double() - exact).abs()
        ratio = (err / tol.clamp(min=1e-300)).max().item()
        print("%s: max err / tol %.3g" % (name, ratio))
        assert (err <= tol).all()


@requires_gpu
@pytest.mark.parametrize("name", list(SHAPES))
def test_backward_deterministic_and_strides(name):
    r = _case(name)
    assert _bit_equal(r["dw"], r["dw2"]) and _bit_equal(r["db"], r["db2"])
    assert r["dw"].stride() == r["w"].stride() == (27, 9, 3, 1)
    assert r["dw_cl"].stride() == (27, 1, 9, 3)
    assert _bit_equal(r["dw_cl"], r["dw"]) and _bit_equal(r["db_cl"], r["db"])


# --- exact cases -----------------------------------------------------------

def _exact_weights():
    k = torch.arange(27).view(1, 27)
    co = torch.arange(64).view(64, 1)
    # 27 distinct integers in -13 .. 13 per output channel
    w = ((k * 5 + co) % 27 - 13).view(64, 3, 3, 3).double()
    b = ((torch.arange(64) % 17) - 8).double() * 0.25
    return w, b


# (n, y, x) in a (2, 9, 40) image: corners, edges, interior, and pixels on
# both sides of a tile boundary
POSITIONS = [(0, 0, 0), (1, 8, 39), (0, 0, 17), (1, 5, 0), (1, 4, 20),
             (0, 3, 31), (0, 4, 32)]


@requires_gpu
@pytest.mark.parametrize("channels_last_weight", [False, True])
def test_forward_one_hot_exact(channels_last_weight):
    w, b = _exact_weights()
    wb = w.bfloat16()
    if channels_last_weight:
        wb = wb.contiguous(**CL)
    for i, (n, py, px) in enumerate(POSITIONS):
        x = torch.zeros(2, 3, 9, 40, dtype=torch.float64)
        x[n, i % 3, py, px] = 1.0
        ref = torch.relu(F.conv2d(x, w, b, 1, 1)).bfloat16()
        assert torch.equal(ref.double(),
                           torch.relu(F.conv2d(x, w, b, 1, 1)))  # exact
        y = _fwd(x.bfloat16().contiguous(**CL), wb, b.bfloat16())
        assert _bit_equal(y, ref), (n, py, px)


@requires_gpu
@pytest.mark.parametrize("channels_last_weight", [False, True])
def test_backward_one_hot_exact(channels_last_weight):
    gen = torch.Generator().manual_seed(5)
    x = torch.randint(-9, 10, (2, 3, 9, 40), generator=gen).double()
    xb = x.bfloat16().contiguous(**CL)
    like = torch.empty(64, 3, 3, 3, dtype=torch.bfloat16)
    if channels_last_weight:
        like = like.contiguous(**CL)
    y = torch.ones(2, 64, 9, 40).bfloat16().contiguous(**CL)
    for i, (n, py, px) in enumerate(POSITIONS):
        g = torch.zeros(2, 64, 9, 40, dtype=torch.float64)
        g[n, (11 * i + 3) % 64, py, px] = 2.0
        dw, db = _bwd(g.bfloat16().contiguous(**CL), y, xb, like)
        assert dw.stride() == like.stride()
        assert _bit_equal(dw, _wgrad64(x, g).bfloat16()), (n, py, px)
        assert _bit_equal(db, g.sum((0, 2, 3)).bfloat16())


@requires_gpu
def test_nan_and_negative_zero():
    """As in test_gpu_conv_epilogue.py: ReLU keeps a NaN (0x7FC0), the
    backward passes g where !(y <= 0), so a NaN y passes and -0.0 does not,
    and a -0.0 or NaN gradient goes through as it is."""
    w, b = _exact_weights()
    x = torch.zeros(1, 3, 6, 35, dtype=torch.float64)
    x[0, 1, 2, 33] = float("nan")
    y = _fwd(x.bfloat16().contiguous(**CL), w.bfloat16(), b.bfloat16()).cpu()
    nan = torch.zeros(1, 1, 6, 35, dtype=torch.bool)
    nan[0, 0, 1:4, 32:35] = True
    assert torch.equal(torch.isnan(y), nan.expand_as(y))
    assert (_bits(y)[nan.expand_as(y)] == 0x7FC0).all()
    ref = torch.relu(b).bfloat16().view(1, 64, 1, 1).expand_as(y)
    assert torch.equal(_bits(y)[~torch.isnan(y)], _bits(ref)[~torch.isnan(y)])

    # exact backward: small integers, sums below 256
    gen = torch.Generator().manual_seed(9)
    vals = torch.tensor([float("nan"), -0.0, 0.0, -1.0, 2.0])
    yb = vals[torch.randint(0, 5, (2, 64, 5, 7), generator=gen)]
    yb = yb.bfloat16().contiguous(**CL)
    gvals = torch.tensor([-1.0, -0.0, 0.0, 1.0])
    g = gvals[torch.randint(0, 4, (2, 64, 5, 7), generator=gen)]
    g[1, 5, 2, 3] = float("nan")
    yb[1, 5, 2, 3] = 2.0
    g = g.bfloat16().contiguous(**CL)
    xs = torch.randint(-2, 3, (2, 3, 5, 7), generator=gen).double()
    dx = torch.ops.aten.threshold_backward(g, yb, 0)
    assert (dx[torch.isnan(yb)] == g[torch.isnan(yb)]).all()
    dw, db = _bwd(g, yb, xs.bfloat16().contiguous(**CL),
                  torch.empty(64, 3, 3, 3, dtype=torch.bfloat16))
    dw_ref = _wgrad64(xs, dx.double()).bfloat16()
    db_ref = dx.double().sum((0, 2, 3)).bfloat16()
    assert torch.isnan(dw_ref[5]).all() and torch.isnan(db_ref[5])
    assert torch.isnan(dw[5]).all() and torch.isnan(db[5])
    keep = torch.arange(64) != 5
    assert _bit_equal(dw[keep], dw_ref[keep])
    assert _bit_equal(db[keep], db_ref[keep])


@requires_gpu
def test_negative_zero_preactivation():
    """A -0.0 pre-activation: x is a single 2^-70 and the weights are
    +-2^-70, so the f32 sum is +-2^-140 at the nine pixels the tap reaches
    (or a zero of that sign, should the matrix unit flush it); either rounds
    to a bf16 zero of its sign. Everywhere else the sum is +0.0: zeros of
    both signs added to the accumulator's +0.0. Bias and ReLU must then do
    what epi_bias_relu_kernel does with those pre-activations, bit for
    bit, with biases of -0.0, +0.0 and +-0.25."""
    tiny = 2.0 ** -70
    gen = torch.Generator().manual_seed(13)
    sign = torch.randint(0, 2, (64, 3, 3, 3), generator=gen).double() * 2 - 1
    b = torch.tensor([-0.0, 0.0, 0.25, -0.25]).repeat(16).bfloat16()
    x = torch.zeros(1, 3, 6, 35, dtype=torch.float64)
    x[0, 2, 3, 31] = 1.0
    pre_sign = F.conv2d(x, sign, None, 1, 1)
    assert (pre_sign < 0).any() and (pre_sign > 0).any()
    pre = torch.where(pre_sign < 0, -0.0, 0.0).bfloat16().contiguous(**CL)
    assert torch.signbit(pre).any()
    ref = pre.cuda()
    _lib().conv_bias_relu_(ref, b.cuda())
    y = _fwd((x * tiny).bfloat16().contiguous(**CL), (sign * tiny).bfloat16(),
             b)
    assert _bit_equal(y, ref)


@requires_gpu
def test_backward_nan_at_image_edge():
    """A NaN in the image's last row and column, in a tile that reaches
    beyond the image: it must spoil exactly the taps that see it. The
    tile's pixels outside the image have dx = 0; their patches must be
    zero too, not the NaN next to them."""
    gen = torch.Generator().manual_seed(17)
    n, h, wd = 1, TH + 1, TW + 1
    x = torch.randint(-1, 2, (n, 3, h, wd), generator=gen).double()
    x[0, 1, h - 1, wd - 1] = float("nan")
    g = torch.randint(-1, 2, (n, 64, h, wd), generator=gen).double()
    g[g == 0] = 1.0  # every pixel contributes, so the NaN shows at its taps
    y = torch.ones(n, 64, h, wd).bfloat16().contiguous(**CL)
    dw, db = _bwd(g.bfloat16().contiguous(**CL), y,
                  x.bfloat16().contiguous(**CL),
                  torch.empty(64, 3, 3, 3, dtype=torch.bfloat16))
    ref = _wgrad64(x, g)
    nan = torch.isnan(ref)
    # channel 1, and only the taps whose pixel lies in the image
    want = torch.zeros(3, 3, 3, dtype=torch.bool)
    want[1, 1:, 1:] = True
    assert torch.equal(nan, want.expand(64, 3, 3, 3))
    dw = dw.cpu()
    assert torch.equal(torch.isnan(dw), nan)
    assert torch.equal(_bits(dw)[~nan], _bits(ref.bfloat16())[~nan])
    assert _bit_equal(db, g.sum((0, 2, 3)).bfloat16())


# --- model level -----------------------------------------------------------

def _prefix():
    from bagua_amd.models.vgg import VGG, _CFGS

    torch.manual_seed(21)
    with torch.device("cuda"):
        model = VGG(_CFGS["D"][:6], num_classes=10)
    return model.bfloat16().to(**CL)


def _prefix_grads(model, x, monkeypatch):
    """Gradients of the features' parameters, and x, y and dL/dy of the
    first stage as whichever path ran it saw them."""
    from bagua_amd.ops import conv_epilogue, first_conv

    seen = {}

    def watch(y, path):
        if "y" not in seen:
            seen["y"], seen["path"] = y, path
            y.register_hook(lambda g: seen.__setitem__("g", g))
        return y

    real_new = first_conv.first_conv_bias_relu
    real_old = conv_epilogue.conv_bias_relu
    monkeypatch.setattr(
        first_conv, "first_conv_bias_relu",
        lambda *a: watch(real_new(*a), "first_conv"))
    monkeypatch.setattr(
        conv_epilogue, "conv_bias_relu",
        lambda c, b, pool=False, tbg=False: (
            real_old(c, b, pool, tbg) if pool or "y" in seen
            else watch(real_old(c, b, pool, tbg), "conv_epilogue")))
    model.zero_grad()
    out = model._features(x)
    out.float().square().sum().backward()
    return [p.grad.clone() for p in model.features.parameters()], seen


def _layer1_exact(x, seen):
    """float64 weight and bias gradient of the first stage from the y and
    dL/dy one path had, each with its bound (module docstring)"""
    y, g = seen["y"].detach().cpu(), seen["g"].cpu()
    dx64 = torch.where(y <= 0, torch.zeros_like(g), g).double()
    x64 = x.cpu().double()
    p = x.shape[0] * x.shape[2] * x.shape[3]
    out = []
    for exact, first in (
            (_wgrad64(x64, dx64),
             p * 2.0 ** -24 * _wgrad64(x64.abs(), dx64.abs())),
            (dx64.sum((0, 2, 3)),
             p * 2.0 ** -24 * dx64.abs().sum((0, 2, 3)))):
        out.append((exact, first + 2.0 ** -8 * (exact.abs() + first)))
    return out


# Gradients of the two paths, relative in the 2-norm per parameter. Behind
# y1 the two runs are the same code on inputs that differ by bf16 roundings.
# From y1 to a parameter gradient a value passes at most 12 tensors that
# are rounded to bf16 (6 forward: three convolution outputs and their
# bias + ReLU; 5 backward: dL/dout and four dx; the gradient itself), and
# two bf16 roundings of nearly the same number are at most one step,
# 2^-7 relative, apart. To first order the steps add: 12 * 2^-7 < 2^-3.
# ReLU and pool decisions that flip are not in this count; it is an
# estimate of rounding noise, set before any measurement, not a proof. A
# transposed, shifted or mis-scaled first stage is off by order 1.
GRAD_REL_BOUND = 2.0 ** -3


# 16x16 is the size this check is set at. MIOpen's pick for so small an image
# varies from job to job: it has rounded a fifth of y1 one bf16 step away
# from this kernel, and it has agreed bitwise. At 17x70 it has agreed at all
# but one element, so the same assertions bind far tighter there.
@requires_gpu
@pytest.mark.parametrize("shape", [(2, 16, 16), (3, 17, 70)])
def test_vgg16_prefix_against_existing_path(monkeypatch, shape):
    """VGG16's features up to the second pool, fused first stage against
    the existing path (conv2d, then the fused epilogue):

    * y1 of the two paths, at every element: the kernel rounds the f32 sum
      to nearest (half a bf16 step, sum within e of s), the existing
      convolution is taken to round faithfully (under one step), so the
      convolution outputs are at most 1.5 steps of |s| + e and 2e apart;
      the bias add rounds each to nearest, one more step of the sum;
      ReLU does not widen it. A step is at most 2^-7 of the value.
    * the first stage's gradients of each path within the module's bound
      of float64 from that path's own y1 and dL/dy1;
    * every parameter's gradient against the existing path within
      GRAD_REL_BOUND."""
    n, h, wd = shape
    model = _prefix()
    gen = torch.Generator().manual_seed(22)
    x = torch.randn(n, 3, h, wd, generator=gen).bfloat16().cuda()
    x = x.contiguous(**CL)
    new, seen = _prefix_grads(model, x, monkeypatch)
    assert seen["path"] == "first_conv"
    model.torch_bias_grad = True  # the switch keeps the existing path
    old, seen_old = _prefix_grads(model, x, monkeypatch)
    assert seen_old["path"] == "conv_epilogue"

    conv = model.features[0]
    x64 = x.cpu().double()
    w64 = conv.weight.detach().cpu().double()
    b64 = conv.bias.detach().cpu().double().view(1, -1, 1, 1)
    s = F.conv2d(x64, w64, None, 1, 1)
    e = 32 * 2.0 ** -24 * F.conv2d(x64.abs(), w64.abs(), None, 1, 1)
    allowed_y = 2.0 ** -7 * (2.5 * (s.abs() + e) + b64.abs()) + 2 * e
    y_new = seen["y"].detach().cpu()
    y_old = seen_old["y"].detach().cpu()
    dy = (y_new.double() - y_old.double()).abs()
    ndiff = (_bits(y_new) != _bits(y_old)).sum().item()
    print("%s: y1 differs at %d of %d elements, max |diff| / allowed %.3g"
          % (shape, ndiff, y_new.numel(),
             (dy / allowed_y.clamp(min=1e-300)).max().item()))

    ex_new, ex_old = _layer1_exact(x, seen), _layer1_exact(x, seen_old)
    own = []
    for i, name in enumerate(("weight", "bias")):
        a, r = new[i].cpu().double(), old[i].cpu().double()
        (en, tn), (eo, to) = ex_new[i], ex_old[i]
        print("first stage %s: new err/bound %.3g, existing err/bound %.3g"
              % (name, ((a - en).abs() / tn).max().item(),
                 ((r - eo).abs() / to).max().item()))
        own.append((a - en).abs() <= tn)
    rel = []
    for a, r in zip(new, old):
        a, r = a.double(), r.double()
        rel.append(((a - r).norm() / r.norm()).item())
        print("parameter %s: |new - existing| / |existing| = %.3g"
              % (tuple(a.shape), rel[-1]))

    assert (dy <= allowed_y).all()
    for ok in own:
        assert ok.all()
    assert len(rel) == 8 and all(v <= GRAD_REL_BOUND for v in rel)


@requires_gpu
def test_hooked_first_conv_keeps_existing_path(monkeypatch):
    model = _prefix()
    x = torch.randn(2, 3, 16, 16).bfloat16().cuda().contiguous(**CL)
    shapes = []
    model.features[0].register_forward_hook(
        lambda m, i, o: shapes.append(tuple(o.shape)))
    _, seen = _prefix_grads(model, x, monkeypatch)
    # the hooked conv runs as a module; first_conv is not asked at all
    assert seen.get("path") != "first_conv"
    assert shapes == [(2, 64, 16, 16)]


@requires_gpu
def test_graph_capture_and_replay():
    from bagua_amd.ops import first_conv

    r = _case("small")
    w = r["w"].cuda().requires_grad_()
    b = r["b"].cuda().requires_grad_()
    xs = torch.zeros_like(r["x"], device="cuda")
    gs = torch.zeros_like(r["g"], device="cuda")

    def run():
        y = first_conv.first_conv_bias_relu(xs, w, b)
        return (y,) + torch.autograd.grad(y, (w, b), gs)

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
    xs.copy_(r["x"])
    gs.copy_(r["g"])
    graph.replay()
    torch.cuda.synchronize()
    assert _bit_equal(outs[0], r["y"])
    assert _bit_equal(outs[1], r["dw"]) and _bit_equal(outs[2], r["db"])
