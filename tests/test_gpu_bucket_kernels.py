"""Bucket and optimizer kernels of ops/csrc/kernels.hip at edge shapes,
against float64 references computed from the exact input values.

Sizes are derived from the launcher constants so that vector bodies,
scalar tails, wire padding and the second grid-stride iteration are all
reached. Bounds are derived, not tuned: wherever the arithmetic allows it
the check is bitwise, otherwise

    |out - ref64| <= k * eps32 * mag + half_ulp_T(ref64)

with ``mag`` the sum of the absolute values of the formula's terms in
float64 and ``k`` the number of f32 roundings in the kernel's expression
(counted from the source, written beside each use; casts of double
arguments to float, ``rsqrtf``, a reciprocal multiply and a possible FMA
contraction count one each). Every rounding is really at most eps32/2 of
its sub-expression, so the form has a factor two in hand for second-order
terms. The helper functions are plain torch and device-agnostic, so the
same formulas evaluated with f32 torch ops can be pushed through them on
a CPU. GPU-only."""

import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

DTYPES = [torch.float32, torch.float16, torch.bfloat16]
EPS32 = 2.0 ** -23

# launcher constants (ops/csrc/kernels.hip)
BLOCK = 256
MAX_GRID = 2048
COMPRESS_CAP = 512  # MINMAX_MAX_BLOCKS, also the decompress cap


def _vec(dtype):
    """Vec16<T>::N, elements per 16-byte vector."""
    return 4 if dtype == torch.float32 else 8


def _grid_for(work_items, cap=MAX_GRID):
    return max(1, min(cap, (work_items + BLOCK - 1) // BLOCK))


def _grid_cap_size(per_iter, launch_div, cap=MAX_GRID):
    """Size at which a launcher ``grid_for(n / launch_div + 1)`` capped at
    ``cap`` blocks reaches the cap AND the grid-stride loop over
    ``n / per_iter`` vector items takes a second iteration in some
    threads only, plus an odd scalar tail."""
    threads = cap * BLOCK
    n_cap = launch_div * (cap - 1) * BLOCK   # smallest n with grid == cap
    n_two = per_iter * (threads + 1000)      # 1000 threads iterate twice
    n = max(n_cap, n_two) + 5                # + scalar tail
    assert _grid_for(n // launch_div + 1, cap) == cap
    assert threads < n // per_iter < 2 * threads
    assert n % per_iter != 0
    return n


def _name(dtype):
    return str(dtype).replace("torch.", "")


def _bits_equal(a, b):
    """Bitwise equality (NaN payloads and signed zeros included)."""
    return torch.equal(a.contiguous().view(torch.uint8),
                       b.contiguous().view(torch.uint8))


def _half_ulp(ref64, dtype):
    """Half a unit in the last place of ``dtype`` at ref64 (0 for f32:
    its roundings are what k counts)."""
    if dtype == torch.float32:
        return torch.zeros_like(ref64)
    # mantissa bits, exponent of the smallest normal
    p, emin = (10, -14) if dtype == torch.float16 else (7, -126)
    _, ex = torch.frexp(ref64)               # |ref| = m * 2**ex, m in [.5, 1)
    e = torch.where(ref64 == 0, torch.full_like(ex, emin), ex - 1)
    e = e.clamp(min=emin)
    return torch.ldexp(torch.ones_like(ref64), e - (p + 1))


def _assert_close(out, ref64, mag64, k, what):
    bound = k * EPS32 * mag64 + _half_ulp(ref64, out.dtype)
    err = (out.double() - ref64).abs()
    ratio = torch.where(bound > 0, err / bound,
                        torch.where(err > 0, torch.full_like(err, 1e30),
                                    torch.zeros_like(err)))
    i = int(ratio.argmax())
    print("BOUND %s k=%d n=%d: worst err %.3e at bound %.3e (%.3f of it)"
          % (what, k, out.numel(), float(err[i]), float(bound[i]),
             float(ratio[i])))
    assert bool((err <= bound).all()), (
        "%s: |out-ref64| = %.6e > bound %.6e at index %d (k=%d)"
        % (what, float(err[i]), float(bound[i]), i, k))


def _randn(n, dtype, seed, scale=1.0):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return (torch.randn(n, device="cuda", generator=g) * scale).to(dtype)


# ---------------------------------------------------------------------------
# 1. elementwise ops and async_model_average
# ---------------------------------------------------------------------------

def _ew_refs(x, y, r, c):
    """(name, ref64, mag64, k) of every elementwise op, from the exact
    inputs. Shared with the CPU self-check of the bounds."""
    xd, yd, rd, cd = x.double(), y.double(), r.double(), c.double()
    ax, ay = xd.abs(), yd.abs()
    return [
        # (x + y) * 0.5f: one add; the multiply by 0.5 is exact
        ("average", (xd + yd) * 0.5, (ax + ay) * 0.5, 1),
        ("add", xd + yd, ax + ay, 1),
        ("sub", xd - yd, ax + ay, 1),
        # x + y * f: cast of f, multiply, add
        ("addmul0.37", xd + yd * 0.37, ax + ay * 0.37, 3),
        ("addmul-1.5", xd + yd * -1.5, ax + ay * 1.5, 3),
        # x * (1.0f / 3.0f): reciprocal, multiply
        ("divide3", xd / 3.0, ax / 3.0, 2),
        # x + r * (1.0f / 4.0f) - c: reciprocal, multiply, add, subtract
        ("async_avg4", xd + rd / 4.0 - cd, ax + rd.abs() / 4.0 + cd.abs(), 4),
    ]


def _ew_call(_C, name, a, y, r, c):
    if name == "average":
        _C.average_inplace(a, y)
    elif name == "add":
        _C.add_inplace(a, y)
    elif name == "sub":
        _C.substract_inplace(a, y)
    elif name == "addmul0.37":
        _C.addmul_inplace(a, y, 0.37)
    elif name == "addmul-1.5":
        _C.addmul_inplace(a, y, -1.5)
    elif name == "divide3":
        _C.divide_inplace(a, 3.0)
    else:
        _C.async_model_average(a, r, c, 4.0)


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("n", [1, 7, 8, 9, 15, 16, 17, 33, 4097, "cap"])
def test_elementwise_vs_float64(dtype, n):
    from bagua_amd import _C

    v = _vec(dtype)
    if n == "cap":
        # ew_kernel: 2 vectors per thread-iteration, grid_for(n/(2V)+1);
        # f32 gives 8*2048*256 + 8*1000 + 5, the half types 16 in place of 8
        n = _grid_cap_size(2 * v, 2 * v)
        # async_avg_kernel: 1 vector per iteration, grid_for(n/4 + 1)
        n_async = _grid_cap_size(v, 4)
        assert n_async <= n
    else:
        n_async = n
    x, y = _randn(n, dtype, 100), _randn(n, dtype, 101)
    r, c = _randn(n, dtype, 102), _randn(n, dtype, 103)
    y0, r0, c0 = y.clone(), r.clone(), c.clone()
    for name, ref, mag, k in _ew_refs(x, y, r, c):
        m = n_async if name == "async_avg4" else n
        a = x[:m].clone()
        _ew_call(_C, name, a, y[:m], r[:m], c[:m])
        _assert_close(a, ref[:m], mag[:m], k,
                      "%s %s" % (name, _name(dtype)))
        assert _bits_equal(y, y0), "%s wrote to y" % name
        assert _bits_equal(r, r0), "%s wrote to reduced" % name
        assert _bits_equal(c, c0), "%s wrote to x_copy" % name


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_elementwise_special_values(dtype):
    """inf + -inf = NaN, NaN propagates, f16 60000 + 60000 = inf; in the
    vector body (first 16/32 elements) and in the scalar tail alike."""
    from bagua_amd import _C

    inf, nan = float("inf"), float("nan")
    xs = [inf, nan, 1.0, 60000.0, -inf, 2.5, -60000.0, inf]
    ys = [-inf, 1.0, nan, 60000.0, -inf, 0.5, -60000.0, 3.0]
    v2 = 2 * _vec(dtype)
    # body: the specials, then ordinary values up to 2 vectors; scalar
    # tail: inf + -inf, NaN + 1, 1 + NaN, 60000 + 60000, -inf + -inf
    fill = [0.25 * i for i in range(v2 - len(xs))]
    x = torch.tensor(xs + fill + xs[:5], device="cuda").to(dtype)
    y = torch.tensor(ys + fill + ys[:5], device="cuda").to(dtype)
    assert x.numel() == v2 + 5
    for op, fn in [("add", lambda a, b: a + b), ("sub", lambda a, b: a - b),
                   ("average", lambda a, b: (a + b) * 0.5)]:
        a = x.clone()
        _ew_call(_C, op, a, y, None, None)
        ref = fn(x.float(), y.float()).to(dtype)
        assert torch.equal(torch.isnan(a), torch.isnan(ref)), op
        assert torch.equal(torch.isposinf(a), torch.isposinf(ref)), op
        assert torch.equal(torch.isneginf(a), torch.isneginf(ref)), op
        fin = torch.isfinite(ref)
        assert torch.equal(a[fin], ref[fin]), op
    if dtype == torch.float16:
        a = x.clone()
        _C.add_inplace(a, y)
        assert bool(torch.isposinf(a[3])) and bool(torch.isneginf(a[6]))


# ---------------------------------------------------------------------------
# 2. reduce_chunk
# ---------------------------------------------------------------------------

def _reduce_ref(x, num_chunks, average):
    """ref64, mag64, k of reduce_chunk: num_chunks - 1 adds (the first
    lands on 0), the reciprocal 1.0f / num_chunks and the multiply by
    it: k = num_chunks + 1."""
    v = x.double().view(num_chunks, -1)
    post = 1.0 / num_chunks if average else 1.0
    return v.sum(0) * post, v.abs().sum(0) * post, num_chunks + 1


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("num_chunks,chunk",
                         [(1, 9), (3, 1), (3, 7), (8, 4099), (2, "cap")])
def test_reduce_chunk_vs_float64(dtype, num_chunks, chunk):
    from bagua_amd import _C

    if chunk == "cap":
        # reduce_chunk_kernel: 1 vector per iteration, grid_for(chunk/4+1)
        chunk = _grid_cap_size(_vec(dtype), 4)
    x = _randn(num_chunks * chunk, dtype, 200)
    for average in (True, False):
        ref, mag, k = _reduce_ref(x, num_chunks, average)
        for target in sorted({0, num_chunks - 1}):
            out = x.clone()
            _C.reduce_chunk_inplace(out, num_chunks, target, average)
            ov, xv = out.view(num_chunks, -1), x.view(num_chunks, -1)
            _assert_close(ov[target], ref, mag, k,
                          "reduce_chunk %s" % _name(dtype))
            for c in range(num_chunks):
                if c != target:
                    assert _bits_equal(ov[c], xv[c]), (
                        "chunk %d changed (target %d)" % (c, target))


# ---------------------------------------------------------------------------
# 3.-5. compress
# ---------------------------------------------------------------------------

def _oracle_wire(x, num_chunks):
    """The pure-torch oracle on the CPU, fed the exact values as f32."""
    from bagua_amd.ops import quant

    return quant.compress_chunked(x.float().cpu(), num_chunks)


def _gpu_wire(x, num_chunks, fill, target=-1):
    from bagua_amd import _C
    from bagua_amd.ops import quant

    chunk = x.numel() // num_chunks
    stride = quant.compressed_chunk_bytes(chunk)
    wire = torch.full((stride * num_chunks,), fill, dtype=torch.uint8,
                      device="cuda")
    _C.compress_chunked(x, wire, num_chunks, target)
    torch.cuda.synchronize()
    return wire.cpu(), stride


def _describe_wire_diff(got, want, stride, chunk):
    i = int((got != want).nonzero()[0])
    c, off = divmod(i, stride)
    part = ("header" if off < 8 else "header tail" if off < 32 else
            "payload" if off < 32 + chunk else "padding")
    return ("wire differs from the oracle in %d bytes; first at byte %d = "
            "chunk %d %s offset %d: got %d, oracle %d"
            % (int((got != want).sum()), i, c, part, off, int(got[i]),
               int(want[i])))


def _planted(num_chunks, chunk, dtype, seed):
    """randn*3 chunks with the extremes planted where a dropped scalar
    tail or a dropped block would lose them: chunk 0 has its maximum at
    element 0 and its minimum at the last element, the last chunk has
    both in the middle."""
    x = _randn(num_chunks * chunk, dtype, seed, 3.0).view(num_chunks, chunk)
    if chunk >= 3:
        x[0, 0], x[0, chunk - 1] = 20.0, -20.0
        if num_chunks > 1:
            x[-1, chunk // 2], x[-1, chunk // 2 - 1] = 24.0, -24.0
    return x.reshape(-1)


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("num_chunks,chunk",
                         [(1, 1), (3, 3), (3, 31), (3, 33), (3, 1001),
                          (8, 4099), (2, "cap")])
def test_compress_wire_bitwise(dtype, num_chunks, chunk):
    """The whole wire (header, header tail, payload, padding) equals the
    oracle's, for every dtype: the inputs are exact in f32 and both sides
    do the same f32 operations."""
    if chunk == "cap":
        # minmax_/quantize_kernel: 1 vector per iteration, gx =
        # min(grid_for(chunk/8 + 1), 512): gx reaches 512, so
        # minmax_finalize_kernel (256 threads) loops twice as well
        chunk = _grid_cap_size(_vec(dtype), 8, COMPRESS_CAP)
    x = _planted(num_chunks, chunk, dtype, 300)
    want = _oracle_wire(x, num_chunks)
    got, stride = _gpu_wire(x, num_chunks, 0xFF)
    assert torch.equal(got, want), _describe_wire_diff(got, want, stride,
                                                       chunk)


def _f32_scale(mn, mx):
    """quant_params' scale = 255.0f / (mx - mn + 1e-7f): one correctly
    rounded f32 division (a Python scalar over a tensor would be
    reciprocal-then-multiply in torch, 1 ulp off now and then)."""
    d = mx - mn + 1e-7
    return torch.full_like(d, 255.0) / d


def _roundtrip_bound(xc, minmax):
    """(0.5 + 2*eps32*M*scale)/scale + 2*eps32*M per chunk, M = max|x|:
    half a level, plus the f32 rounding of x*scale, of level-lower and of
    the decode, which grow with M*scale when |mean| >> range."""
    mn, mx = minmax[0], minmax[1]
    scale = _f32_scale(mn, mx).double()
    M = xc.double().abs().max()
    return (0.5 + 2 * EPS32 * M * scale) / scale + 2 * EPS32 * M


def _edge_chunks(chunk):
    """name -> one chunk of f32 values (CPU). Shared with tests/test_quant."""
    g = torch.Generator()
    g.manual_seed(400)
    return {
        "zero": torch.zeros(chunk),
        "const1": torch.ones(chunk),
        "const-3.7": torch.full((chunk,), -3.7),
        "offset1000": 1000 + 1e-3 * torch.rand(chunk, generator=g),
        "offset-1e4": -1e4 + 1e-1 * torch.rand(chunk, generator=g),
        "tiny1e-20": torch.randn(chunk, generator=g) * 1e-20,
        "huge1e30": torch.randn(chunk, generator=g) * 1e30,
    }


# where the values survive the cast (offsets collapse to a constant in
# the half types, 1e-20 underflows f16, 1e30 is asked for f32 only)
_EDGE_DTYPES = {
    "zero": DTYPES, "const1": DTYPES, "const-3.7": DTYPES,
    "offset1000": [torch.float32], "offset-1e4": [torch.float32],
    "tiny1e-20": [torch.float32, torch.bfloat16],
    "huge1e30": [torch.float32],
}


@requires_gpu
@pytest.mark.parametrize("edge,dtype",
                         [(e, d) for e, ds in _EDGE_DTYPES.items()
                          for d in ds],
                         ids=lambda v: v if isinstance(v, str) else _name(v))
def test_compress_edge_inputs(edge, dtype):
    from bagua_amd import _C

    chunk, num_chunks, at = 4099, 3, 1   # edge chunk between randn chunks
    x = _randn(num_chunks * chunk, dtype, 401, 3.0).view(num_chunks, chunk)
    x[at] = _edge_chunks(chunk)[edge].to(dtype).cuda()
    x = x.reshape(-1)
    want = _oracle_wire(x, num_chunks)
    got, stride = _gpu_wire(x, num_chunks, 0xFF)
    assert torch.equal(got, want), _describe_wire_diff(got, want, stride,
                                                       chunk)
    # round trip through the native decompress, into f32 so that the
    # bound needs no output-rounding term
    y = torch.empty(num_chunks * chunk, device="cuda")
    _C.decompress_chunked(got.cuda(), y, num_chunks, -1)
    xc, yc = x.float().cpu().view(num_chunks, -1), y.cpu().view(num_chunks, -1)
    for c in range(num_chunks):
        minmax = want[c * stride:c * stride + 8].view(torch.float32)
        bound = _roundtrip_bound(xc[c], minmax)
        err = (xc[c].double() - yc[c].double()).abs().max()
        print("BOUND roundtrip %s %s chunk %d: err %.3e bound %.3e"
              % (edge, _name(dtype), c, float(err), float(bound)))
        assert err <= bound, "chunk %d: %g > %g" % (c, err, bound)


@requires_gpu
def test_compress_nan_inf_stay_in_their_chunk():
    chunk, num_chunks = 1001, 4
    x = _randn(num_chunks * chunk, torch.float32, 402, 3.0)
    x[17] = float("nan")
    x[chunk + 1000] = float("inf")
    want = _oracle_wire(x, num_chunks)
    got, stride = _gpu_wire(x, num_chunks, 0xFF)
    for c in (2, 3):
        assert torch.equal(got[c * stride:(c + 1) * stride],
                           want[c * stride:(c + 1) * stride]), c


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_target_chunk_paths(dtype):
    from bagua_amd import _C

    chunk, num_chunks = 1001, 4
    x = _planted(num_chunks, chunk, dtype, 500)
    full, stride = _gpu_wire(x, num_chunks, 0xFF)
    for t in (0, num_chunks - 1):
        only, _ = _gpu_wire(x, num_chunks, 0xAB, target=t)
        lo, hi = t * stride, (t + 1) * stride
        assert torch.equal(only[lo:hi], full[lo:hi]), "target %d region" % t
        rest = torch.cat([only[:lo], only[hi:]])
        assert bool((rest == 0xAB).all()), "target %d wrote elsewhere" % t

        flat = _randn(num_chunks * chunk, dtype, 501)
        keep = flat.clone()
        _C.decompress_chunked(full.cuda(), flat, num_chunks, t)
        alld = torch.empty_like(flat)
        _C.decompress_chunked(full.cuda(), alld, num_chunks, -1)
        fv, kv = flat.view(num_chunks, -1), keep.view(num_chunks, -1)
        assert _bits_equal(fv[t], alld.view(num_chunks, -1)[t])
        for c in range(num_chunks):
            if c != t:
                assert _bits_equal(fv[c], kv[c]), (
                    "decompress target %d wrote chunk %d" % (t, c))


# ---------------------------------------------------------------------------
# 6. decompress
# ---------------------------------------------------------------------------

def _decompress_ref(wire, num_chunks, chunk, stride):
    """float64 (q + lower) / scale per chunk, with scale and lower the f32
    numbers the wire format defines (quant.decompress computes them with
    the same f32 operations as quant_params). k = 3: q + lower, the
    reciprocal 1.0f / scale, the multiply by it."""
    refs, mags = [], []
    for c in range(num_chunks):
        hdr = wire[c * stride:c * stride + 8].view(torch.float32)
        scale = _f32_scale(hdr[0], hdr[1])
        lower = torch.round(hdr[1] * scale) - 255.0
        q = wire[c * stride + 32:c * stride + 32 + chunk].double()
        refs.append((q + lower.double()) / scale.double())
        mags.append((q + lower.double().abs()) / scale.double())
    return torch.cat(refs), torch.cat(mags), 3


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("num_chunks,chunk",
                         [(1, 1), (3, 3), (3, 31), (3, 33), (3, 1001),
                          (8, 4099)])
def test_decompress_vs_float64(dtype, num_chunks, chunk):
    from bagua_amd import _C
    from bagua_amd.ops import quant

    x = _planted(num_chunks, chunk, torch.float32, 600)
    wire = _oracle_wire(x, num_chunks)
    stride = quant.compressed_chunk_bytes(chunk)
    ref, mag, k = _decompress_ref(wire, num_chunks, chunk, stride)
    y = torch.empty(num_chunks * chunk, dtype=dtype, device="cuda")
    _C.decompress_chunked(wire.cuda(), y, num_chunks, -1)
    _assert_close(y.cpu(), ref, mag, k, "decompress %s" % _name(dtype))


# ---------------------------------------------------------------------------
# 7. dequant_reduce
# ---------------------------------------------------------------------------

@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("chunk", [16, 33, 4099])
@pytest.mark.parametrize("num_chunks", [1, 2, 8, 64, 65])
def test_dequant_reduce_bitwise(dtype, chunk, num_chunks):
    """Fused kernel == decompress then reduce_chunk, bitwise; 65 chunks
    take the unfused fallback of ops.dequant_reduce. Only the target
    chunk of flat is written on either path."""
    from bagua_amd import ops

    flat = _randn(num_chunks * chunk, dtype, 700, 3.0)
    wire = ops.compress_chunked(flat, num_chunks)
    dec = torch.empty_like(flat)
    ops.decompress_chunked_into(wire, dec, num_chunks)
    for average in (True, False):
        for target in sorted({0, num_chunks - 1}):
            a = dec.clone()
            ops.reduce_chunk_inplace(a, num_chunks, target, average)
            b = flat.clone()
            ops.dequant_reduce(wire, b, num_chunks, target, average)
            av, bv = a.view(num_chunks, -1), b.view(num_chunks, -1)
            assert _bits_equal(av[target], bv[target]), (
                "fused deviates by %g" % (av[target].float()
                                          - bv[target].float()).abs().max())
            fv = flat.view(num_chunks, -1)
            for c in range(num_chunks):
                if c != target:
                    assert _bits_equal(bv[c], fv[c]), (
                        "chunk %d of flat changed (target %d)" % (c, target))


# ---------------------------------------------------------------------------
# 8. fused SGD / Adam / mixed SGD, through _C on flat tensors
# ---------------------------------------------------------------------------

def _sgd_ref(p, g, m, lr, mu, damp, wd, nesterov, initialized):
    """One torch.optim.SGD step in float64 from the exact f32 inputs.
    Returns (p_ref, p_mag, k_p, m_ref, m_mag, k_m)."""
    pd, gd, md = p.double(), g.double(), m.double()
    grad = gd + wd * pd
    grad_mag = gd.abs() + wd * pd.abs()
    # g + wd * p: cast of wd, multiply, add
    k_grad = 3 if wd != 0 else 0
    if mu != 0:
        if initialized:
            buf = mu * md + (1 - damp) * grad
            buf_mag = mu * md.abs() + (1 - damp) * grad_mag
            # mu*m + (1-damp)*grad: casts of mu and damp, the subtraction,
            # two multiplies, add
            k_buf = k_grad + 6
        else:
            buf, buf_mag, k_buf = grad, grad_mag, k_grad
        if nesterov:
            upd = grad + mu * buf
            upd_mag = grad_mag + mu * buf_mag
            # grad + mu * buf: cast of mu, multiply, add
            k_upd = k_grad + k_buf + 3
        else:
            upd, upd_mag, k_upd = buf, buf_mag, k_buf
    else:
        buf, buf_mag, k_buf = md, md.abs(), 0
        upd, upd_mag, k_upd = grad, grad_mag, k_grad
    # p - lr * upd: cast of lr, multiply, subtract
    return (pd - lr * upd, pd.abs() + lr * upd_mag, k_upd + 3,
            buf, buf_mag, k_buf)


_SGD_VARIANTS = [
    # momentum, dampening, nesterov
    ("plain", 0.0, 0.0, False),
    ("momentum", 0.9, 0.0, False),
    ("nesterov", 0.9, 0.0, True),
    ("dampening", 0.9, 0.1, False),
]


def _sgd_size(n):
    # fused_sgd_kernel / _mixed_ / fused_adam_kernel: 8 elements per
    # thread-iteration, grid_for(n/8 + 1)
    return _grid_cap_size(8, 8) if n == "cap" else n


@requires_gpu
@pytest.mark.parametrize("n", [1, 7, 8, 9, 4099, "cap"])
def test_fused_sgd_vs_float64(n):
    from bagua_amd import _C

    n = _sgd_size(n)
    lr = 0.05
    for name, mu, damp, nesterov in _SGD_VARIANTS:
        for wd in (0.0, 1e-2):
            p = _randn(n, torch.float32, 800)
            m = _randn(n, torch.float32, 801)   # junk until initialized
            for step in range(3):
                g = _randn(n, torch.float32, 810 + step)
                g0 = g.clone()
                m_before = m.clone()
                (p_ref, p_mag, k_p, m_ref, m_mag, k_m) = _sgd_ref(
                    p, g, m, lr, mu, damp, wd, nesterov, step > 0)
                _C.fused_sgd_step(p, g, m, lr, mu, damp, wd, nesterov,
                                  step > 0)
                what = "sgd %s wd=%g step %d" % (name, wd, step)
                _assert_close(p, p_ref, p_mag, k_p, what + " p")
                if mu != 0:
                    _assert_close(m, m_ref, m_mag, k_m, what + " m")
                else:
                    assert _bits_equal(m, m_before), "momentum=0 wrote m"
                assert _bits_equal(g, g0)


@requires_gpu
@pytest.mark.parametrize("n", [1, 7, 8, 9, 4099, "cap"])
def test_fused_sgd_mixed_vs_float64(n):
    """bf16 params and grads, f32 master and momentum: p is the bf16
    rounding of the new master, bitwise."""
    from bagua_amd import _C

    n = _sgd_size(n)
    lr = 0.05
    for name, mu, damp, nesterov in _SGD_VARIANTS:
        for wd in (0.0, 1e-2):
            master = _randn(n, torch.float32, 820)
            p = master.bfloat16()
            m = _randn(n, torch.float32, 821)
            for step in range(3):
                g = _randn(n, torch.bfloat16, 830 + step)
                m_before = m.clone()
                (w_ref, w_mag, k_w, m_ref, m_mag, k_m) = _sgd_ref(
                    master, g, m, lr, mu, damp, wd, nesterov, step > 0)
                _C.fused_sgd_mixed_step(p, g, master, m, lr, mu, damp, wd,
                                        nesterov, step > 0)
                what = "sgd_mixed %s wd=%g step %d" % (name, wd, step)
                _assert_close(master, w_ref, w_mag, k_w, what + " master")
                assert torch.equal(p, master.bfloat16()), what
                if mu != 0:
                    _assert_close(m, m_ref, m_mag, k_m, what + " m")
                else:
                    assert _bits_equal(m, m_before), "momentum=0 wrote m"


def _adam_ref(p, g, m, v, step, lr, beta1, beta2, eps, wd, adamw):
    """One torch.optim.Adam / AdamW step in float64 from the exact f32
    inputs. Returns [(name, ref, mag, k)] for p, m, v."""
    pd, gd, md, vd = p.double(), g.double(), m.double(), v.double()
    if adamw:
        param = pd * (1 - lr * wd)
        param_mag = pd.abs() * (1 + lr * wd)
        # p * (1 - lr*wd): casts of lr and wd, multiply, subtract, multiply
        k_param = 5 if wd != 0 else 0
        grad, grad_mag, k_grad = gd, gd.abs(), 0
    else:
        param, param_mag, k_param = pd, pd.abs(), 0
        grad = gd + wd * pd
        grad_mag = gd.abs() + wd * pd.abs()
        # g + wd * p: cast of wd, multiply, add
        k_grad = 3 if wd != 0 else 0
    mi = beta1 * md + (1 - beta1) * grad
    mi_mag = beta1 * md.abs() + (1 - beta1) * grad_mag
    # beta1*m + (1-beta1)*grad: cast of beta1, the subtraction, two
    # multiplies, add
    k_m = k_grad + 5
    vi = beta2 * vd + (1 - beta2) * grad * grad
    vi_mag = beta2 * vd.abs() + (1 - beta2) * grad_mag * grad_mag
    # beta2*v + (1-beta2)*grad*grad: as above plus one multiply; grad
    # enters squared, so its error counts twice
    k_v = 2 * k_grad + 6
    bc1 = 1 - beta1 ** step
    bc2 = 1 - beta2 ** step
    denom = vi.sqrt() / bc2 ** 0.5 + eps
    # sqrtf(vi)*rsqrtf(bc2) + eps: cast of bc2, rsqrtf, sqrtf, multiply,
    # cast of eps, add, plus half of vi's relative error (vi is a sum of
    # non-negative terms when v >= 0, so it has no cancellation)
    k_denom = 6 + (k_v + 1) // 2
    # ... unless weight decay cancels inside grad: k_v counts against
    # vi_mag, so the update term carries vi_mag / vi (1 without decay)
    amp = torch.where(vi > 0, vi_mag / vi, torch.ones_like(vi))
    upd_mag = lr / bc1 * mi_mag / denom * amp
    # param - lr * (1/bc1) * mi / denom: casts of lr and bc1, reciprocal,
    # two multiplies, divide, subtract
    k_p = k_param + 7 + k_m + k_denom
    return [("p", param - lr / bc1 * mi / denom, param_mag + upd_mag, k_p),
            ("m", mi, mi_mag, k_m), ("v", vi, vi_mag, k_v)]


@requires_gpu
@pytest.mark.parametrize("n", [1, 7, 8, 9, 4099, "cap"])
def test_fused_adam_vs_float64(n):
    """Parameters are small next to lr so that the bound on p is governed
    by the update term: an error in the bias corrections must not hide
    behind eps32 * |p|."""
    from bagua_amd import _C

    n = _sgd_size(n)
    lr, eps = 1e-2, 1e-8
    for adamw, wd in ((False, 0.0), (False, 1e-2), (True, 1e-2)):
        for beta2 in (0.999, 0.95):
            for step in (1, 2, 10):
                p = _randn(n, torch.float32, 840, 1e-3)
                g = _randn(n, torch.float32, 841)
                if step == 1:
                    m = torch.zeros_like(p)
                    v = torch.zeros_like(p)
                else:
                    m = _randn(n, torch.float32, 842, 0.3)
                    v = _randn(n, torch.float32, 843, 0.3).square()
                refs = _adam_ref(p, g, m, v, step, lr, 0.9, beta2, eps, wd,
                                 adamw)
                _C.fused_adam_step(p, g, m, v, step, lr, 0.9, beta2, eps,
                                   wd, adamw)
                for (name, ref, mag, k), out in zip(refs, (p, m, v)):
                    _assert_close(out, ref, mag, k,
                                  "adam%s wd=%g beta2=%g step %d %s"
                                  % ("w" if adamw else "", wd, beta2, step,
                                     name))


# ---------------------------------------------------------------------------
# 9. offset views
# ---------------------------------------------------------------------------

@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_offset_views_match_aligned(dtype):
    """x starting 1 and 3 elements into its allocation (2..12 bytes off
    the 16-byte vector alignment) gives the results of the aligned run."""
    from bagua_amd import _C
    from bagua_amd.ops import quant

    num_chunks, chunk = 3, 1001
    n = num_chunks * chunk
    x, y = _planted(num_chunks, chunk, dtype, 900), _randn(n, dtype, 901)
    stride = quant.compressed_chunk_bytes(chunk)

    def run(xin):
        a = xin
        wire = torch.full((stride * num_chunks,), 0xFF, dtype=torch.uint8,
                          device="cuda")
        _C.compress_chunked(a, wire, num_chunks, -1)
        _C.addmul_inplace(a, y, 0.37)
        ew = a.clone()
        _C.reduce_chunk_inplace(a, num_chunks, num_chunks - 1, True)
        return wire, ew, a.clone()

    want = run(x.clone())
    for off in (1, 3):
        base = torch.zeros(n + 8, dtype=dtype, device="cuda")
        view = base[off:off + n]
        view.copy_(x)
        got = run(view)
        for w, gt, what in zip(want, got, ("compress", "addmul", "reduce")):
            assert _bits_equal(w, gt), "%s at offset %d" % (what, off)
        assert bool((base[:off] == 0).all()) and \
            bool((base[off + n:] == 0).all()), "wrote outside the view"
