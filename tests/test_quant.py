"""MinMaxUInt8 quantizer numerics vs the golden formula
(reference semantics: tests/internal/compressor.py:4-33)."""

import pytest
import torch

from bagua_amd.ops import quant


def _golden_compress(tensor):
    eps, levels = 1e-7, 255.0
    _min, _max = torch.min(tensor), torch.max(tensor)
    scale = levels / (_max - _min + eps)
    upper = torch.round(_max * scale)
    lower = upper - levels
    level = torch.clamp(torch.round(tensor * scale), max=upper)
    return _min, _max, (level - lower).to(torch.uint8)


def test_roundtrip_error_bound():
    torch.manual_seed(0)
    x = torch.rand(1000)
    minmax, payload = quant.compress(x)
    y = quant.decompress(minmax, payload)
    # quantization step = range/255; roundtrip error <= one step
    step = (x.max() - x.min()) / 255.0
    assert (x - y).abs().max() <= step + 1e-6


def test_matches_golden():
    torch.manual_seed(1)
    x = torch.randn(4096)
    _min, _max, gold = _golden_compress(x)
    minmax, payload = quant.compress(x)
    assert torch.equal(payload, gold)
    assert torch.allclose(minmax[0], _min) and torch.allclose(minmax[1], _max)


def test_chunked_wire_roundtrip():
    torch.manual_seed(2)
    n_chunks = 4
    x = torch.randn(n_chunks * 256)
    buf = quant.compress_chunked(x, n_chunks)
    y = quant.decompress_chunked(buf, n_chunks, 256)
    step = (x.view(n_chunks, -1).max(1).values
            - x.view(n_chunks, -1).min(1).values).max() / 255.0
    assert (x - y).abs().max() <= step + 1e-6


def test_chunked_target_chunk():
    torch.manual_seed(3)
    n_chunks = 4
    x = torch.randn(n_chunks * 64)
    full = quant.compress_chunked(x, n_chunks)
    only2 = quant.compress_chunked(x, n_chunks, target_chunk=2)
    stride = quant.compressed_chunk_bytes(64)
    assert torch.equal(full[2 * stride:3 * stride],
                       only2[2 * stride:3 * stride])
    assert only2[:stride].sum() == 0  # untouched chunks stay zero


# ---------------------------------------------------------------------------
# ill-conditioned chunks: constant, |mean| >> range, tiny, huge. In f32
# level - lower leaves [0, 255] there; unclamped, the uint8 cast wraps.
# ---------------------------------------------------------------------------

EPS32 = 2.0 ** -23


def _edge_inputs(n=4096):
    g = torch.Generator()
    g.manual_seed(400)
    return {
        "zero": torch.zeros(n),
        "const1": torch.ones(n),
        "const-3.7": torch.full((n,), -3.7),
        "ones64": torch.ones(64),
        "offset1000": 1000 + 1e-3 * torch.rand(n, generator=g),
        "offset-1e4": -1e4 + 1e-1 * torch.rand(n, generator=g),
        "tiny1e-20": torch.randn(n, generator=g) * 1e-20,
        "huge1e30": torch.randn(n, generator=g) * 1e30,
        "randn": torch.randn(n, generator=g) * 3,
    }


def _f32_levels(x):
    """level - lower exactly as compress() forms it, before any cast."""
    _min, _max = x.min(), x.max()
    d = _max - _min + 1e-7
    scale = torch.full_like(d, 255.0) / d   # one division, not 255 * (1/d)
    upper = torch.round(_max * scale)
    lower = upper - 255.0
    return torch.clamp(torch.round(x * scale), max=upper) - lower, scale


@pytest.mark.parametrize("name", sorted(_edge_inputs()))
def test_edge_input_levels_do_not_wrap(name):
    x = _edge_inputs()[name]
    q, _ = _f32_levels(x)
    _, payload = quant.compress(x)
    # the payload is the f32 level saturated to [0, 255], never wrapped
    assert torch.equal(payload.int(), q.clamp(0, 255).int())


@pytest.mark.parametrize("name", sorted(_edge_inputs()))
def test_edge_input_roundtrip_bound(name):
    """err <= (0.5 + 2*eps32*M*scale)/scale + 2*eps32*M, M = max|x|: half
    a level, plus the f32 roundings of x*scale, level-lower and the
    decode, which grow with M*scale when |mean| >> range."""
    x = _edge_inputs()[name]
    minmax, payload = quant.compress(x)
    y = quant.decompress(minmax, payload)
    _, scale = _f32_levels(x)
    scale, M = scale.double(), x.double().abs().max()
    bound = (0.5 + 2 * EPS32 * M * scale) / scale + 2 * EPS32 * M
    err = (x.double() - y.double()).abs().max()
    assert err <= bound, "%s: %g > %g" % (name, err, bound)


def test_chunked_out_region_fully_written():
    """A caller-supplied wire: every byte of a written chunk region is
    defined (header tail and padding zero), other regions untouched."""
    torch.manual_seed(4)
    n_chunks, chunk = 3, 33
    x = torch.randn(n_chunks * chunk)
    stride = quant.compressed_chunk_bytes(chunk)
    full = quant.compress_chunked(x, n_chunks)
    out = torch.full((stride * n_chunks,), 0xAB, dtype=torch.uint8)
    quant.compress_chunked(x, n_chunks, target_chunk=1, out=out)
    assert torch.equal(out[stride:2 * stride], full[stride:2 * stride])
    assert (out[:stride] == 0xAB).all() and (out[2 * stride:] == 0xAB).all()


def test_scale_is_one_division():
    """scale is the correctly rounded quotient 255/d like the kernel's
    ``255.0f / d``; ``255.0 / tensor`` in torch is reciprocal-then-multiply
    and 1 ulp off for about a quarter of all ranges. At |x|*scale > 2**24
    that ulp moves every level by 2."""
    x = _edge_inputs()["offset-1e4"]
    d = x.max() - x.min() + 1e-7
    exact = 255.0 / d.double()
    scale = quant._scale(x.min(), x.max())
    assert scale.dtype == torch.float32
    assert scale.double() == exact.float().double()
