"""The gfx950 dropout + residual add + LayerNorm kernels
(csrc/layernorm_kernels.hip) behind ``contrib.FusedDropoutAddLayerNorm``:
against float64 with the torch chain as the yardstick, the dropout mask,
determinism, and BERT's use of them. GPU-only."""

import copy
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from bagua_amd.contrib import FusedDropoutAddLayerNorm
from bagua_amd.models.bert import BertForPretrainingShape, bert_tiny
from bagua_amd.ops import layernorm as ln_ops

pytestmark = pytest.mark.gpu
requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
# name: (dtype of x, of h (None: no branch), of the parameters (None: none),
# R, H, p)
CASES = {
    # one chunk and one mask byte; autocast's dtypes with a second iteration
    # of a single lane; BERT's row; plain LayerNorm; the longest row;
    # grid-stride with a tail and several rows per lane in backward; rows
    # far from zero, where a one-pass variance cancels
    "one_chunk": (BF16, BF16, BF16, 1, 8, 0.25),
    "autocast": (F32, BF16, F32, 3, 520, 0.1),
    "bert_row": (F16, F16, F32, 5, 1024, 0.1),
    "plain": (F32, None, None, 4, 128, 0.0),
    "hmax": (BF16, BF16, F32, 2, ln_ops.HMAX, 0.1),
    "grid_stride": (F32, F32, F32,
                    2 * ln_ops.WAVES_PER_BLOCK * ln_ops.FWD_MAX_GRID + 5, 64,
                    0.1),
    "far_mean": (F32, F32, F32, 4, 1024, 0.1),
}
CASES.update({n + "_p0": c[:5] + (0.0,) for n, c in list(CASES.items())
              if c[5] > 0})
NAMES = sorted(CASES)
EPS = 1e-5


def _make(name):
    tx, th, tp, rows, hidden, p = CASES[name]
    gen = torch.Generator().manual_seed(sum(map(ord, name)) * 7919)

    def rand(*shape):
        return torch.randn(*shape, generator=gen)

    x = rand(rows, hidden) * 2 + 0.5
    if name.startswith("far_mean"):
        x = rand(rows, hidden) + 1000.0
    d = dict(x=x.to(tx).cuda(), g=rand(rows, hidden).to(tx).cuda())
    if th is not None:
        d["h"] = rand(rows, hidden).to(th).cuda()
    if tp is not None:
        d["gamma"] = (1 + 0.5 * rand(hidden)).to(tp).cuda()
        d["beta"] = (0.5 * rand(hidden)).to(tp).cuda()
        if th is not None:
            d["b"] = (0.5 * rand(hidden)).to(tp if tp == F32 else th).cuda()
    return d, p


def _chain(d, p, keep, dtype=None):
    """``y`` and the gradients of the written-out formula under ``keep``, in
    the tensors' own dtypes or all in ``dtype``."""
    t = {k: (v if dtype is None else v.to(dtype)).clone().requires_grad_()
         for k, v in d.items() if k != "g"}
    s = t["x"]
    if "h" in t:
        branch = t["h"]
        if "b" in t:  # a Linear's output: rounded to its dtype after the bias
            branch = (branch + t["b"]).to(branch.dtype)
        s = s + branch * keep.to(branch.dtype) / (1 - p)
    gamma, beta = t.get("gamma"), t.get("beta")
    if gamma is not None and gamma.dtype != s.dtype:  # as autocast runs it
        y = F.layer_norm(s.float(), s.shape[-1:], gamma, beta, EPS)
        y = y.to(s.dtype)
    else:
        y = F.layer_norm(s, s.shape[-1:], gamma, beta, EPS)
    keys = [k for k in t]
    grads = torch.autograd.grad(y, [t[k] for k in keys], d["g"].to(y.dtype))
    return dict(zip(("d" + k for k in keys), grads), y=y.detach())


def _module_step(d, p, seed):
    ln = FusedDropoutAddLayerNorm(d["x"].shape[-1],
                                  elementwise_affine="gamma" in d).cuda()
    if "gamma" in d:
        ln.weight.data, ln.bias.data = d["gamma"].clone(), d["beta"].clone()
    t = {k: v.clone().requires_grad_() for k, v in d.items()
         if k in ("x", "h", "b")}
    torch.manual_seed(seed)
    y = ln(t["x"], t.get("h"), t.get("b"), p)
    t.update(dict(ln.named_parameters()))
    names = dict(weight="gamma", bias="beta")
    grads = torch.autograd.grad(y, list(t.values()), d["g"])
    return dict(zip(("d" + names.get(k, k) for k in t), grads), y=y.detach())


@functools.lru_cache(maxsize=None)
def _runs(name):
    """Kernels through the module (twice), the torch chain and float64 under
    the kernels' own mask; shared, read-only."""
    d, p = _make(name)
    assert ln_ops.kernels_apply(d["x"], d["x"].shape[-1:], d.get("h"),
                                d.get("b"), d.get("gamma"), d.get("beta"), p)
    torch.manual_seed(7)  # the seed the module will draw
    out = ln_ops.forward(d["x"], d.get("h"), d.get("b"), d.get("gamma"),
                         d.get("beta"), p, EPS)
    mask = out[4]
    keep = torch.ones_like(d["x"])
    if mask is not None:
        keep = ((mask.unsqueeze(-1) >> torch.arange(8, device="cuda")) & 1
                ).reshape(d["x"].shape).to(d["x"].dtype)
    got, again = _module_step(d, p, 7), _module_step(d, p, 7)
    assert torch.equal(got["y"], out[0])
    res = dict(d=d, p=p, out=out, keep=keep, got=got, again=again,
               chain=_chain(d, p, keep), ref=_chain(d, p, keep, torch.float64))
    torch.cuda.synchronize()
    return res


@requires_gpu
@pytest.mark.parametrize("name", NAMES)
def test_against_float64(name):
    """The rule of test_gpu_syncbn_act_kernels.py: at most twice the torch
    chain's error plus half an ulp at the reference's largest magnitude."""
    r = _runs(name)
    assert r["got"].keys() == r["chain"].keys() == r["ref"].keys()
    for key, ref in r["ref"].items():
        got, chain = r["got"][key], r["chain"][key]
        assert got.shape == ref.shape and got.dtype == chain.dtype
        assert torch.isfinite(ref).all()
        fi = torch.finfo(got.dtype)
        top = max(ref.abs().max().item(), fi.tiny)
        half_ulp = 0.5 * fi.eps * 2.0 ** math.floor(math.log2(top))
        err = (got.double() - ref).abs().max().item()
        err_base = (chain.double() - ref).abs().max().item()
        print("%s %s: kernels %.3g, yardstick %.3g, half ulp %.3g, ratio "
              "%.3g" % (name, key, err, err_base, half_ulp,
                        err / err_base if err_base else float("inf")))
        assert err <= 2 * err_base + half_ulp, key


@requires_gpu
@pytest.mark.parametrize("name", NAMES)
def test_determinism_and_shared_gradient(name):
    r = _runs(name)
    for key, t in r["got"].items():
        assert torch.equal(t.view(torch.uint8),
                           r["again"][key].view(torch.uint8)), key
    d, p = r["d"], r["p"]
    _, s, mean, rstd, mask = r["out"]
    assert (mask is None) == (p == 0)
    if p == 0 and "h" in d:  # dh is ds: one tensor when the dtypes agree
        dx, dh = ln_ops.backward(d["g"], s, mean, rstd, d.get("gamma"), None,
                                 0.0, d["h"].dtype)[:2]
        assert (dh is dx) == (d["h"].dtype == d["x"].dtype)
    if p > 0 and d["x"].dtype == F32:  # dropped: s is x, to the bit
        assert torch.equal(s[r["keep"] == 0], d["x"][r["keep"] == 0])


@requires_gpu
def test_mask_is_a_function_of_seed_and_index():
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(128, 1024, generator=gen).cuda()
    h = torch.randn(128, 1024, generator=gen).cuda()
    seed = torch.tensor([1234567890123], device="cuda")

    def mask(rows, seed):
        return ln_ops.forward(x[:rows], h[:rows], None, None, None, 0.1, EPS,
                              seed)[4]

    m = mask(64, seed)
    assert m.dtype == torch.uint8 and m.shape == (64, 128)
    assert torch.equal(m, mask(64, seed))
    assert not torch.equal(m, mask(64, seed + 1))
    assert torch.equal(m, mask(128, seed)[:64])  # the counter, not the launch
    kept = sum(((m >> k) & 1).sum().item() for k in range(8)) / 65536
    print("kept share %.5f" % kept)
    assert abs(kept - 0.9) <= 5 * math.sqrt(0.1 * 0.9 / 65536)


@requires_gpu
def test_declined_above_hmax_runs_the_torch_chain():
    hidden = ln_ops.HMAX + 8
    gen = torch.Generator().manual_seed(2)
    x = torch.randn(2, hidden, generator=gen).to(BF16).cuda()
    h = torch.randn(2, hidden, generator=gen).to(BF16).cuda()
    ln = FusedDropoutAddLayerNorm(hidden).cuda().to(BF16)
    assert not ln_ops.kernels_apply(x, (hidden,), h, None, ln.weight,
                                    ln.bias, 0.0)
    want = F.layer_norm(x + h, (hidden,), ln.weight, ln.bias, ln.eps)
    assert torch.equal(ln(x, h), want)


@requires_gpu
def test_bert_tiny_takes_the_kernels(monkeypatch):
    calls = dict(forward=0, backward=0)
    for key in calls:
        def counted(*a, _f=getattr(ln_ops, key), _k=key, **kw):
            calls[_k] += 1
            return _f(*a, **kw)
        monkeypatch.setattr(ln_ops, key, counted)
    torch.manual_seed(0)
    model = bert_tiny().cuda().train()
    ids = torch.randint(0, 1024, (2, 24), device="cuda")
    with torch.autocast("cuda", dtype=BF16):
        start, end = model(ids)
    (start.float().square().sum() + end.float().sum()).backward()
    assert calls == dict(forward=9, backward=9)  # 2 per layer + embedding
    for n, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
    assert model.layers[0].attn.out.bias.grad.abs().max() > 0
    assert model.layers[0].mlp[2].bias.grad.abs().max() > 0

    model.eval()
    outs = {}
    with torch.no_grad():
        ref = copy.deepcopy(model).double()(ids)
        for flag in (True, False):
            monkeypatch.setattr(BertForPretrainingShape, "fuse_add_ln", flag)
            with torch.autocast("cuda", dtype=BF16):
                outs[flag] = model(ids)
    assert calls["forward"] == 18
    for got, base, want in zip(outs[True], outs[False], ref):
        fi = torch.finfo(got.dtype)
        top = max(want.abs().max().item(), fi.tiny)
        half_ulp = 0.5 * fi.eps * 2.0 ** math.floor(math.log2(top))
        err = (got.double() - want).abs().max().item()
        err_base = (base.double() - want).abs().max().item()
        print("bert_tiny eval: fused %.3g, modules %.3g, half ulp %.3g"
              % (err, err_base, half_ulp))
        assert err <= 2 * err_base + half_ulp
