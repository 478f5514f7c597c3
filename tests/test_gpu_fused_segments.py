"""Segmented fused optimizer steps (ops/csrc/kernels.hip
fused_segments_kernel) against the flat kernels, through ``_C``.

The segmented entry points read each gradient where it lives; everything
else is the flat step. So on a gathered copy of the same gradients the
flat call must give the same parameters, master and state bit for bit,
whatever the segment layout does to the kernel's paths:

* flat offsets at every residue mod 8 (vectors that straddle segments),
* gradient addresses that are 16-byte aligned, or not,
* a missing gradient (None: a zero gradient),
* more segments than one launch's table holds (several launches, whose
  ranges begin and end inside a flat vector),
* a segment longer than one pass of the grid.

One float64 check per optimizer ties the pair to torch's formulas, with
the bounds of tests/test_gpu_bucket_kernels.py: k roundings of size
eps32 * (sum of the magnitudes of the terms).
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

EPS32 = 2.0 ** -23

# launcher constants (ops/csrc/kernels.hip)
BLOCK = 256
MAX_GRID = 2048
SEG_CAP = 128

NUMELS = [1, 7, 8, 9, 64, 1000, 4099]
LAYOUTS = ["separate", "bucket", "bucket_shifted", "none_middle",
           "over_capacity", "long_segment"]

_SGD_VARIANTS = [
    # momentum, dampening, nesterov
    ("plain", 0.0, 0.0, False),
    ("momentum", 0.9, 0.0, False),
    ("nesterov", 0.9, 0.0, True),
    ("dampening", 0.9, 0.1, False),
]


def _bits_equal(a, b):
    """Bitwise equality (NaN payloads and signed zeros included)."""
    return torch.equal(a.contiguous().view(torch.uint8),
                       b.contiguous().view(torch.uint8))


def _randn(n, dtype, seed, scale=1.0):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return (torch.randn(n, device="cuda", generator=g) * scale).to(dtype)


def _numels(layout):
    if layout == "over_capacity":
        # 1..9 elements each, three segments more than one table holds
        return [1 + (5 * k) % 9 for k in range(SEG_CAP + 3)]
    if layout == "long_segment":
        # every thread of a full grid takes a vector, 512 take a second
        # one, and 3 elements are left for the scalar path
        return [MAX_GRID * BLOCK * 8 + 4099]
    return NUMELS


def _grads(layout, dtype, seed):
    """(grads, offsets, gathered): the gradient tensors as the segmented
    call takes them and the same values in one flat tensor."""
    numels = _numels(layout)
    total = sum(numels)
    offsets = [0]
    for n in numels:
        offsets.append(offsets[-1] + n)
    flat = _randn(total, dtype, seed)
    if layout in ("bucket", "bucket_shifted"):
        # one shared buffer, the tensors laid out in reverse order; the
        # shift by one element moves every view off the alignment it has
        # in the unshifted run
        shift = 1 if layout == "bucket_shifted" else 0
        buf = torch.empty(total + shift, dtype=dtype, device="cuda")
        assert buf.data_ptr() % 16 == 0
        buf = buf[shift:]
        grads, end = [], total
        for k, n in enumerate(numels):
            view = buf[end - n:end]
            view.copy_(flat[offsets[k]:offsets[k + 1]])
            grads.append(view)
            end -= n
    else:
        # every gradient its own allocation
        grads = [flat[offsets[k]:offsets[k + 1]].clone()
                 for k in range(len(numels))]
    if layout == "none_middle":
        mid = len(numels) // 2
        grads[mid] = None
        flat[offsets[mid]:offsets[mid + 1]] = 0
    return grads, offsets, flat


def _check_grads_untouched(grads, before):
    for g, b in zip(grads, before):
        if g is not None:
            assert _bits_equal(g, b), "the step wrote to a gradient"


def _clones(grads):
    return [None if g is None else g.clone() for g in grads]


@requires_gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_sgd_segments_match_flat(layout):
    from bagua_amd import _C

    lr = 0.05
    n = sum(_numels(layout))
    for name, mu, damp, nesterov in _SGD_VARIANTS:
        for wd in (0.0, 1e-2):
            p = _randn(n, torch.float32, 900)
            m = _randn(n, torch.float32, 901)   # junk until initialized
            p_flat, m_flat = p.clone(), m.clone()
            for step in range(3):
                grads, offsets, g = _grads(layout, torch.float32, 910 + step)
                before = _clones(grads)
                _C.fused_sgd_step_segments(p, grads, offsets, m, lr, mu,
                                           damp, wd, nesterov, step > 0)
                _C.fused_sgd_step(p_flat, g, m_flat, lr, mu, damp, wd,
                                  nesterov, step > 0)
                what = "sgd %s wd=%g step %d" % (name, wd, step)
                assert _bits_equal(p, p_flat), what + " p"
                assert _bits_equal(m, m_flat), what + " m"
                _check_grads_untouched(grads, before)


@requires_gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_sgd_mixed_segments_match_flat(layout):
    from bagua_amd import _C

    lr = 0.05
    n = sum(_numels(layout))
    for name, mu, damp, nesterov in _SGD_VARIANTS:
        for wd in (0.0, 1e-2):
            master = _randn(n, torch.float32, 920)
            p = master.bfloat16()
            m = _randn(n, torch.float32, 921)
            master_flat, p_flat, m_flat = master.clone(), p.clone(), m.clone()
            for step in range(3):
                grads, offsets, g = _grads(layout, torch.bfloat16, 930 + step)
                before = _clones(grads)
                _C.fused_sgd_mixed_step_segments(
                    p, grads, offsets, master, m, lr, mu, damp, wd, nesterov,
                    step > 0)
                _C.fused_sgd_mixed_step(p_flat, g, master_flat, m_flat, lr,
                                        mu, damp, wd, nesterov, step > 0)
                what = "sgd_mixed %s wd=%g step %d" % (name, wd, step)
                assert _bits_equal(master, master_flat), what + " master"
                assert _bits_equal(p, p_flat), what + " p"
                assert _bits_equal(m, m_flat), what + " m"
                _check_grads_untouched(grads, before)


@requires_gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_adam_segments_match_flat(layout):
    from bagua_amd import _C

    lr, eps = 1e-2, 1e-8
    n = sum(_numels(layout))
    for adamw, wd in ((False, 0.0), (False, 1e-2), (True, 1e-2)):
        p = _randn(n, torch.float32, 940, 1e-3)
        m = torch.zeros_like(p)
        v = torch.zeros_like(p)
        p_flat, m_flat, v_flat = p.clone(), m.clone(), v.clone()
        for step in (1, 2, 3):
            grads, offsets, g = _grads(layout, torch.float32, 950 + step)
            before = _clones(grads)
            _C.fused_adam_step_segments(p, grads, offsets, m, v, step, lr,
                                        0.9, 0.999, eps, wd, adamw)
            _C.fused_adam_step(p_flat, g, m_flat, v_flat, step, lr, 0.9,
                               0.999, eps, wd, adamw)
            what = "adam%s wd=%g step %d" % ("w" if adamw else "", wd, step)
            assert _bits_equal(p, p_flat), what + " p"
            assert _bits_equal(m, m_flat), what + " m"
            assert _bits_equal(v, v_flat), what + " v"
            _check_grads_untouched(grads, before)


@requires_gpu
def test_segments_are_validated():
    from bagua_amd import _C

    p = torch.zeros(16, device="cuda")
    m = torch.zeros(16, device="cuda")
    g = [torch.zeros(8, device="cuda"), torch.zeros(8, device="cuda")]

    def call(p, g, offsets, m=m):
        _C.fused_sgd_step_segments(p, g, offsets, m, 0.1, 0.9, 0.0, 0.0,
                                   False, True)

    call(p, g, [0, 8, 16])
    with pytest.raises(RuntimeError):   # does not reach numel
        call(p, g[:1], [0, 8])
    with pytest.raises(RuntimeError):   # grad size is not the segment's
        call(p, g, [0, 4, 16])
    with pytest.raises(RuntimeError):   # grad dtype is not the parameters'
        call(p, [g[0], g[1].bfloat16()], [0, 8, 16])
    with pytest.raises(RuntimeError):   # not contiguous
        call(p, [g[0], torch.zeros(16, device="cuda")[::2]], [0, 8, 16])
    with pytest.raises(RuntimeError):   # on the host
        call(p, [g[0], g[1].cpu()], [0, 8, 16])
    with pytest.raises(RuntimeError):   # momentum without a buffer
        call(p, g, [0, 8, 16], m=None)
    with pytest.raises(RuntimeError):   # state of another size
        call(p, g, [0, 8, 16], m=m[:8])


# ---------------------------------------------------------------------------
# float64: the bounds of tests/test_gpu_bucket_kernels.py
# ---------------------------------------------------------------------------

def _assert_close(out, ref64, mag64, k, what):
    """|out - ref64| <= k * eps32 * mag64 for an f32 result of k roundings
    over terms whose magnitudes sum to mag64."""
    assert out.dtype == torch.float32
    bound = k * EPS32 * mag64
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
def test_sgd_segments_vs_float64():
    from bagua_amd import _C

    lr = 0.05
    n = sum(NUMELS)
    for name, mu, damp, nesterov in _SGD_VARIANTS:
        for wd in (0.0, 1e-2):
            p = _randn(n, torch.float32, 960)
            m = _randn(n, torch.float32, 961)
            for step in range(3):
                grads, offsets, g = _grads("separate", torch.float32,
                                           970 + step)
                (p_ref, p_mag, k_p, m_ref, m_mag, k_m) = _sgd_ref(
                    p, g, m, lr, mu, damp, wd, nesterov, step > 0)
                _C.fused_sgd_step_segments(p, grads, offsets, m, lr, mu,
                                           damp, wd, nesterov, step > 0)
                what = "sgd segments %s wd=%g step %d" % (name, wd, step)
                _assert_close(p, p_ref, p_mag, k_p, what + " p")
                if mu != 0:
                    _assert_close(m, m_ref, m_mag, k_m, what + " m")


@requires_gpu
def test_sgd_mixed_segments_vs_float64():
    """bf16 params and grads, f32 master and momentum: p is the bf16
    rounding of the new master, bitwise."""
    from bagua_amd import _C

    lr = 0.05
    n = sum(NUMELS)
    for name, mu, damp, nesterov in _SGD_VARIANTS:
        for wd in (0.0, 1e-2):
            master = _randn(n, torch.float32, 980)
            p = master.bfloat16()
            m = _randn(n, torch.float32, 981)
            for step in range(3):
                grads, offsets, g = _grads("separate", torch.bfloat16,
                                           990 + step)
                (w_ref, w_mag, k_w, m_ref, m_mag, k_m) = _sgd_ref(
                    master, g, m, lr, mu, damp, wd, nesterov, step > 0)
                _C.fused_sgd_mixed_step_segments(
                    p, grads, offsets, master, m, lr, mu, damp, wd, nesterov,
                    step > 0)
                what = "sgd_mixed segments %s wd=%g step %d" % (name, wd,
                                                                step)
                _assert_close(master, w_ref, w_mag, k_w, what + " master")
                assert torch.equal(p, master.bfloat16()), what
                if mu != 0:
                    _assert_close(m, m_ref, m_mag, k_m, what + " m")


@requires_gpu
def test_adam_segments_vs_float64():
    """Parameters are small next to lr so that the bound on p is governed
    by the update term."""
    from bagua_amd import _C

    lr, eps = 1e-2, 1e-8
    n = sum(NUMELS)
    for adamw, wd in ((False, 0.0), (False, 1e-2), (True, 1e-2)):
        for beta2 in (0.999, 0.95):
            for step in (1, 2, 10):
                p = _randn(n, torch.float32, 1000, 1e-3)
                grads, offsets, g = _grads("separate", torch.float32, 1001)
                if step == 1:
                    m = torch.zeros_like(p)
                    v = torch.zeros_like(p)
                else:
                    m = _randn(n, torch.float32, 1002, 0.3)
                    v = _randn(n, torch.float32, 1003, 0.3).square()
                refs = _adam_ref(p, g, m, v, step, lr, 0.9, beta2, eps, wd,
                                 adamw)
                _C.fused_adam_step_segments(p, grads, offsets, m, v, step,
                                            lr, 0.9, beta2, eps, wd, adamw)
                for (name, ref, mag, k), out in zip(refs, (p, m, v)):
                    _assert_close(out, ref, mag, k,
                                  "adam%s segments wd=%g beta2=%g step %d %s"
                                  % ("w" if adamw else "", wd, beta2, step,
                                     name))
