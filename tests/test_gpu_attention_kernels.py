"""The gfx950 attention kernels (csrc/attention_kernels.hip) behind
``contrib.PackedSelfAttention``: against float64 with SDPA as the yardstick,
padded rows, NaN behind the lengths, determinism, declined inputs, and BERT
with ``seq_lens``. GPU-only."""

import functools
import math

import pytest
import torch
import torch.nn.functional as F

from bagua_amd.contrib import PackedSelfAttention
from bagua_amd.models.bert import BertConfig, BertForPretrainingShape
from bagua_amd.ops import attention as att_ops

pytestmark = pytest.mark.gpu
requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

F16, BF16 = torch.float16, torch.bfloat16
HEADS, D = 2, att_ops.HEAD_DIM
H = HEADS * D
BM, BN = att_ops.BLOCK_M, att_ops.BLOCK_N
# name: (dtype, S, lengths (None: two full sequences))
CASES = {
    "ragged": (BF16, 8, None),
    "full_tile": (BF16, BN, None),
    "key_past": (BF16, BN + 1, None),
    "query_past": (BF16, BM + 1, None),
    # a skipped query tile, a length on a tile's edge, a length of one
    "lens": (BF16, 2 * BM + 3, (1, BN, BN + 1)),
    "lens_f16": (F16, 2 * BM + 3, (1, BN, BN + 1)),
    "lens_full": (BF16, 2 * BM + 3, (2 * BM + 3, BM)),
    "bert": (BF16, 384, (384, 200, 65)),
    "zero": (BF16, BN + 1, (0, 5)),
}
NAMES = sorted(CASES)
KEYS = ("out", "dq", "dk", "dv")


def _make(name):
    dtype, S, lens = CASES[name]
    B = 2 if lens is None else len(lens)
    gen = torch.Generator().manual_seed(sum(map(ord, name)) * 7919)
    qkv = torch.randn(B, S, 3 * H, generator=gen).to(dtype).cuda()
    dout = torch.randn(B, S, H, generator=gen).to(dtype).cuda()
    lens_t = None if lens is None else torch.tensor(lens, device="cuda")
    return qkv, dout, lens_t, lens or (S,) * B


def _result(out, dqkv):
    return dict(zip(KEYS, (out.detach(),) + dqkv.split(H, dim=-1)))


def _module_step(qkv, dout, lens_t):
    x = qkv.clone().requires_grad_()
    out = PackedSelfAttention(HEADS)(x, lens_t)
    return _result(out, torch.autograd.grad(out, x, dout)[0])


def _by_slices(qkv, dout, lens, dtype, sdpa):
    """Each sequence's valid rows on their own, in ``dtype``: SDPA, or plain
    softmax attention; zeros behind the lengths."""
    out = torch.zeros(dout.shape, dtype=dtype, device="cuda")
    dqkv = torch.zeros(qkv.shape, dtype=dtype, device="cuda")
    for b, L in enumerate(lens):
        if L == 0:
            continue
        x = qkv[b, :L].to(dtype).requires_grad_()
        q, k, v = x.view(L, 3, HEADS, D).permute(1, 2, 0, 3)  # heads, L, D
        if sdpa:
            y = F.scaled_dot_product_attention(q, k, v)
        else:
            y = torch.softmax(q @ k.transpose(1, 2) / math.sqrt(D), -1) @ v
        y = y.transpose(0, 1).reshape(L, H)
        out[b, :L] = y.detach()
        dqkv[b, :L] = torch.autograd.grad(y, x, dout[b, :L].to(dtype))[0]
    return _result(out, dqkv)


@functools.lru_cache(maxsize=None)
def _runs(name):
    """Kernels through the module (twice, and once with NaN behind the
    lengths), the yardstick and float64; shared, read-only."""
    qkv, dout, lens_t, lens = _make(name)
    assert att_ops.kernels_apply(qkv, HEADS, lens_t)
    pad = (torch.arange(qkv.shape[1], device="cuda")[None, :]
           >= torch.tensor(lens, device="cuda")[:, None])
    nan = float("nan")
    res = dict(
        got=_module_step(qkv, dout, lens_t),
        again=_module_step(qkv, dout, lens_t),
        nan=_module_step(qkv.masked_fill(pad[:, :, None], nan),
                         dout.masked_fill(pad[:, :, None], nan), lens_t),
        chain=_by_slices(qkv, dout, lens, qkv.dtype, True),
        ref=_by_slices(qkv, dout, lens, torch.float64, False), pad=pad)
    torch.cuda.synchronize()
    return res


@requires_gpu
@pytest.mark.parametrize("name", NAMES)
def test_against_float64(name):
    """The rule of the project's kernel tests: at most twice the yardstick's
    error plus half an ulp at the reference's largest magnitude."""
    r = _runs(name)
    for key in KEYS:
        got, chain, ref = r["got"][key], r["chain"][key], r["ref"][key]
        assert got.shape == ref.shape and got.dtype == chain.dtype
        assert torch.isfinite(got).all()
        fi = torch.finfo(got.dtype)
        top = max(ref.abs().max().item(), fi.tiny)
        half_ulp = 0.5 * fi.eps * 2.0 ** math.floor(math.log2(top))
        err = (got.double() - ref).abs().max().item()
        err_base = (chain.double() - ref).abs().max().item()
        print("%s %s: kernels %.3g, yardstick %.3g, half ulp %.3g, ratio %.3g"
              % (name, key, err, err_base, half_ulp,
                 err / err_base if err_base else float("inf")))
        assert err <= 2 * err_base + half_ulp, key


@requires_gpu
@pytest.mark.parametrize("name", NAMES)
def test_padding_nan_and_determinism(name):
    r = _runs(name)
    for key in KEYS:
        got = r["got"][key]
        assert not got[r["pad"]].any(), key  # exactly zero behind a length
        for other in ("again", "nan"):
            assert torch.equal(got.view(torch.int16),
                               r[other][key].view(torch.int16)), (key, other)


@requires_gpu
@pytest.mark.parametrize("what", ["f32", "head_dim_32", "strided"])
def test_declined_runs_the_torch_form(what):
    gen = torch.Generator().manual_seed(5)
    heads = 4 if what == "head_dim_32" else HEADS
    qkv = torch.randn(2, 9, 6 * H, generator=gen).cuda()
    qkv = qkv.to(torch.float32 if what == "f32" else BF16)
    qkv = qkv[:, :, :3 * H] if what == "strided" else \
        qkv[:, :, :3 * H].contiguous()
    lens = torch.tensor([9, 4], device="cuda")
    assert not att_ops.kernels_apply(qkv, heads, lens)
    got = PackedSelfAttention(heads)(qkv, lens)
    assert torch.equal(got, att_ops.reference(qkv, heads, lens))
    assert not got[1, 4:].any()


def _bert_step(model, ids, lens, autocast):
    model.zero_grad()
    with torch.autocast("cuda", dtype=BF16, enabled=autocast):
        start, end = model(ids, lens)
    valid = torch.arange(ids.shape[1], device="cuda")[None, :] < lens[:, None]
    logits = torch.stack([start, end]).float() * valid
    logits.square().sum().backward()
    res = {n: p.grad.float().clone() for n, p in model.named_parameters()}
    res["logits"] = logits.detach()
    return res


@requires_gpu
def test_bert_with_seq_lens(monkeypatch):
    """Kernels against the torch form under bf16 autocast: no further apart
    than MARGIN times what the torch form itself moves between bf16 autocast
    and f32. MARGIN is 1: the kernels round where SDPA rounds, and the step
    to f32 removes the rounding of every other op as well."""
    MARGIN = 1.0
    torch.manual_seed(0)
    model = BertForPretrainingShape(BertConfig(
        vocab_size=1024, hidden_size=H, num_layers=2, num_heads=HEADS,
        intermediate_size=256, max_position=256, dropout=0.0)).cuda().train()
    S = BM + BN + 7
    ids = torch.randint(0, 1024, (3, S), device="cuda")
    lens = torch.tensor([S, BN + 1, 3], device="cuda")
    calls = []
    monkeypatch.setattr(att_ops, "forward", lambda *a, _f=att_ops.forward:
                        calls.append(1) or _f(*a))
    kern = _bert_step(model, ids, lens, True)
    assert len(calls) == 2  # one per layer
    monkeypatch.setattr(att_ops, "kernels_apply", lambda *a: False)
    torch_bf16 = _bert_step(model, ids, lens, True)
    torch_f32 = _bert_step(model, ids, lens, False)
    assert len(calls) == 2
    for key, base in torch_bf16.items():
        spread = (base - torch_f32[key]).abs().max().item()
        err = (kern[key] - base).abs().max().item()
        print("%s: kernels to torch %.3g, bf16 to f32 %.3g" % (key, err,
                                                               spread))
        assert torch.isfinite(kern[key]).all(), key
        assert err <= MARGIN * spread, key
