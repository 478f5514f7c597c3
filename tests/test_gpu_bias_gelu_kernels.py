"""The gfx950 bias + GELU kernels (csrc/bias_gelu_kernels.hip) behind
``contrib.FusedBiasGELU``: against float64 with the torch chain as the
yardstick, determinism, declined inputs, and BERT's use of them. GPU-only."""

import functools
import math

import pytest
import torch
import torch.nn.functional as F

from bagua_amd.contrib import FusedBiasGELU
from bagua_amd.models.bert import BertForPretrainingShape, bert_tiny
from bagua_amd.ops import bias_gelu as bg_ops

pytestmark = pytest.mark.gpu
requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
# name: (dtype of h, of the bias (None: no bias), R, C)
CASES = {
    # one 16-byte vector; a ragged last tile and a wave with idle lanes;
    # several column tiles; f32; plain GELU; one chunk past a column tile;
    # two sweeps of the capped grid and a tail (C = 64: 8 lanes along a row,
    # BLOCK // 8 rows a block); abs(z) up to about 16
    "one_chunk": (BF16, BF16, 1, 8),
    "autocast": (BF16, F32, 3, 520),
    "bert_row": (F16, F32, 5, 4096),
    "f32": (F32, F32, 4, 128),
    "no_bias": (BF16, None, 4, 64),
    "tile_edge": (BF16, F32, 2, bg_ops.TILE_COLS + 8),
    "grid_stride": (F32, F32,
                    2 * (bg_ops.BLOCK // 8) * bg_ops.MAX_GRID + 5, 64),
    "tails": (F32, F32, 4, 256),
}
NAMES = sorted(CASES)
FORMS = ("none", "tanh")


def _make(name):
    th, tb, rows, cols = CASES[name]
    gen = torch.Generator().manual_seed(sum(map(ord, name)) * 7919)
    h = torch.randn(rows, cols, generator=gen) * 1.5
    if name == "tails":
        h *= 16.0 / h.abs().max()
    d = dict(h=h.to(th).cuda(),
             g=torch.randn(rows, cols, generator=gen).to(th).cuda())
    if tb is not None:
        d["b"] = (0.5 * torch.randn(cols, generator=gen)).to(tb).cuda()
    return d


def _chain(d, form, dtype=None):
    """``a`` and the gradients of the torch chain, in the tensors' own dtypes
    (a Linear's output: rounded to its dtype after the bias) or all in
    ``dtype``."""
    t = {k: (v if dtype is None else v.to(dtype)).clone().requires_grad_()
         for k, v in d.items() if k != "g"}
    z = t["h"]
    if "b" in t:
        z = (z + t["b"]).to(z.dtype)
    a = F.gelu(z, approximate=form)
    grads = torch.autograd.grad(a, list(t.values()), d["g"].to(a.dtype))
    return dict(zip(("d" + k for k in t), grads), a=a.detach())


def _module_step(d, form):
    t = {k: v.clone().requires_grad_() for k, v in d.items() if k != "g"}
    a = FusedBiasGELU(approximate=form)(t["h"], t.get("b"))
    grads = torch.autograd.grad(a, list(t.values()), d["g"])
    return dict(zip(("d" + k for k in t), grads), a=a.detach())


@functools.lru_cache(maxsize=None)
def _runs(name, form):
    """Kernels through the module (twice), the torch chain and float64;
    shared, read-only."""
    d = _make(name)
    assert bg_ops.kernels_apply(d["h"], d.get("b"), form)
    res = dict(got=_module_step(d, form), again=_module_step(d, form),
               chain=_chain(d, form), ref=_chain(d, form, torch.float64))
    torch.cuda.synchronize()
    return res


@requires_gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", NAMES)
def test_against_float64(name, form):
    """The rule of test_gpu_syncbn_act_kernels.py: at most twice the torch
    chain's error plus half an ulp at the reference's largest magnitude."""
    r = _runs(name, form)
    assert r["got"].keys() == r["chain"].keys() == r["ref"].keys()
    for key, ref in r["ref"].items():
        got, chain = r["got"][key], r["chain"][key]
        assert got.shape == ref.shape and got.dtype == chain.dtype
        assert torch.isfinite(ref).all() and torch.isfinite(got).all()
        fi = torch.finfo(got.dtype)
        top = max(ref.abs().max().item(), fi.tiny)
        half_ulp = 0.5 * fi.eps * 2.0 ** math.floor(math.log2(top))
        err = (got.double() - ref).abs().max().item()
        err_base = (chain.double() - ref).abs().max().item()
        print("%s %s %s: kernels %.3g, yardstick %.3g, half ulp %.3g, ratio "
              "%.3g" % (name, form, key, err, err_base, half_ulp,
                        err / err_base if err_base else float("inf")))
        assert err <= 2 * err_base + half_ulp, key


@requires_gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", NAMES)
def test_determinism(name, form):
    r = _runs(name, form)
    for key, t in r["got"].items():
        assert torch.equal(t.view(torch.uint8),
                           r["again"][key].view(torch.uint8)), key


@requires_gpu
@pytest.mark.parametrize("what", ["c12", "strided"])
def test_declined_runs_the_torch_chain(what):
    gen = torch.Generator().manual_seed(3)
    cols = 12 if what == "c12" else 64
    h = torch.randn(6, 2 * cols, generator=gen).to(BF16).cuda()
    h = h[:, :cols] if what == "strided" else h[:, :cols].contiguous()
    b = torch.randn(cols, generator=gen).cuda()
    assert not bg_ops.kernels_apply(h, b, "none")
    assert torch.equal(FusedBiasGELU()(h, b), F.gelu(h + b))


@requires_gpu
def test_bert_tiny_takes_the_kernels(monkeypatch):
    calls = dict(forward=0, backward=0)
    for key in calls:
        def counted(*a, _f=getattr(bg_ops, key), _k=key, **kw):
            calls[_k] += 1
            return _f(*a, **kw)
        monkeypatch.setattr(bg_ops, key, counted)
    torch.manual_seed(0)
    model = bert_tiny().cuda().train()
    ids = torch.randint(0, 1024, (2, 24), device="cuda")
    for flag, want in ((True, 4), (False, 0)):  # one call per layer
        monkeypatch.setattr(BertForPretrainingShape, "fuse_bias_gelu", flag)
        calls.update(forward=0, backward=0)
        model.zero_grad()
        with torch.autocast("cuda", dtype=BF16):
            start, end = model(ids)
        (start.float().square().sum() + end.float().sum()).backward()
        assert calls == dict(forward=want, backward=want)
        for n, p in model.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all(), n
        assert model.layers[0].mlp[0].bias.grad.abs().max() > 0
