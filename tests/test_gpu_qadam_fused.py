"""Fused QAdam on the GPU: the momentum-and-wire kernel and the frozen
step against float64, and the whole algorithm against the golden
simulation. Bounds follow tests/test_gpu_bucket_kernels.py."""

import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_bucket_kernels import _assert_close, _bits_equal, _randn

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

BETA1 = 0.9

LAYOUTS = {
    "one": [1],
    "odd": [7, 1, 9],
    "vectors": [8, 8],
    "chunk_edge": [40, 30],       # 40 crosses element 32, a chunk edge
    "padded": [50, 13],           # 63 of 64: one element of padding at least
    "launches": [(7 * i) % 40 + 1 for i in range(130)],  # > SEG_CAP tensors
    # not padded to 32 per chunk: chunks of 12, 4 and 4 elements, so that
    # chunk edges fall inside 8-element vectors
    "ragged": [5, 6],
}


@requires_gpu
@pytest.mark.parametrize("num_chunks", [1, 3, 8])
@pytest.mark.parametrize("layout", list(LAYOUTS) + ["negative"])
def test_momentum_and_wire(layout, num_chunks):
    """Gradient 0 starts 1 element into its allocation, the last of three
    or more is None; the extremes sit on both sides of the first segment
    edge (an element-wise position unless it falls on a multiple of 8).
    "negative": every m is negative, so the padding's 0 is the maximum."""
    from bagua_amd import ops

    negative = layout == "negative"
    numels = LAYOUTS["odd" if negative else layout]
    offsets = [0]
    for n in numels:
        offsets.append(offsets[-1] + n)
    used = offsets[-1]
    align = num_chunks * (4 if layout == "ragged" else 32)
    total = (used + align - 1) // align * align
    m = _randn(total, torch.float32, 1200, 0.3)
    g = _randn(used, torch.float32, 1201)
    if negative:
        m = -m.abs() - 1.0
        g = -g.abs()
        m[used:] = 0.0
    elif len(numels) > 1:
        edge = offsets[1]
        m[edge - 1], g[edge - 1] = 50.0, 50.0
        m[edge], g[edge] = -60.0, -60.0
    grads = []
    for k, n in enumerate(numels):
        if k == 0:
            base = torch.zeros(n + 1, device="cuda")
            base[1:].copy_(g[:n])
            grads.append(base[1:])
        elif len(numels) >= 3 and k == len(numels) - 1:
            g[offsets[k]:] = 0.0
            grads.append(None)
        else:
            grads.append(g[offsets[k]:offsets[k + 1]].clone())
    before = [None if t is None else t.clone() for t in grads]
    m0 = m.clone()
    gfull = torch.zeros(total, device="cuda", dtype=torch.float64)
    gfull[:used] = g.double()
    ref = BETA1 * m.double() + (1 - BETA1) * gfull
    mag = BETA1 * m.double().abs() + (1 - BETA1) * gfull.abs()

    wire = torch.full((ops.compressed_buffer_numel(total, num_chunks),),
                      0xFF, dtype=torch.uint8, device="cuda")
    ops.qadam_momentum_compress_chunked(m, grads, offsets, BETA1, num_chunks,
                                        out=wire)
    # cast of beta1, cast of 1 - beta1, two multiplies, one add
    _assert_close(m, ref, mag, 5, "qadam momentum %s x%d" % (layout,
                                                             num_chunks))
    assert _bits_equal(wire, ops.compress_chunked(m, num_chunks)), \
        "wire differs from compress_chunked of the updated momentum"
    for t, b in zip(grads, before):
        assert t is None or _bits_equal(t, b), "a gradient was written"

    # update-only mode from the same start gives the same momentum
    ops.qadam_momentum_update(m0, grads, offsets, BETA1)
    assert _bits_equal(m0, m), "update-only mode differs"


@requires_gpu
@pytest.mark.parametrize("n", [1, 7, 8, 9, 4099])
def test_frozen_step_vs_float64(n):
    """m split across three allocations, the middle one offset by 1
    element. Small w so that the update term governs the bound."""
    from bagua_amd import _C

    lr, eps = 1e-2, 1e-8
    a = n // 3
    offsets = [0, a, 2 * a, n]
    for beta2 in (0.999, 0.95):
        for step in (4, 50):
            w = _randn(n, torch.float32, 1300, 1e-3)
            m = _randn(n, torch.float32, 1301, 0.3)
            v = _randn(n, torch.float32, 1302, 0.3).square()
            base = torch.zeros(a + 1, device="cuda")
            base[1:].copy_(m[a:2 * a])
            moms = [m[:a].clone(), base[1:], m[2 * a:].clone()]
            v0 = v.clone()
            bc1 = 1 - BETA1 ** step
            bc2 = 1 - beta2 ** step
            denom = v.double().sqrt() / bc2 ** 0.5 + eps
            ref = w.double() - lr / bc1 * m.double() / denom
            mag = w.double().abs() + lr / bc1 * m.double().abs() / denom
            _C.qadam_frozen_step_segments(w, moms, offsets, v, step, lr,
                                          BETA1, beta2, eps)
            # 7 of the update term, 6 of the denominator (see _adam_ref)
            _assert_close(w, ref, mag, 13, "qadam frozen n=%d beta2=%g "
                          "step %d" % (n, beta2, step))
            assert _bits_equal(v, v0), "v was written"
            assert _bits_equal(torch.cat(moms), m), "m was written"


@requires_gpu
def test_fused_qadam_matches_golden_on_gpu():
    from tests import test_qadam_golden as G
    from tests.test_gpu_golden import _setup_env

    _setup_env()
    import bagua_amd
    from bagua_amd.parallel.algorithms import GlobalAlgorithmRegistry
    from bagua_amd.parallel.algorithms.q_adam import FusedQAdamOptimizer

    torch.cuda.set_device(0)
    bagua_amd.init_process_group()

    torch.manual_seed(13)
    model = G.TinyNet().cuda()
    optimizer = FusedQAdamOptimizer(model.parameters(), lr=G.LR,
                                    warmup_steps=G.WARMUP)
    ddp = bagua_amd.DistributedDataParallel(
        model, optimizers=[optimizer],
        algorithm=GlobalAlgorithmRegistry.get("qadam")(optimizer))
    for step in range(G.STEPS):
        data, target = G._data(0, step)
        optimizer.zero_grad()
        loss = F.mse_loss(ddp(data.cuda()), target.cuda())
        loss.backward()
        optimizer.step()
    torch.cuda.synchronize()

    assert ddp.bagua_buckets
    for b in ddp.bagua_buckets:
        assert b._native_idx is not None and len(b.ops) == 1, b.name
    golden = G._simulate(1)[0]
    got = torch.cat([p.detach().reshape(-1).cpu()
                     for p in model.parameters()])
    assert torch.allclose(got, golden, atol=5e-4), (
        "fused GPU QAdam trajectory deviates from golden (max diff %g)"
        % (got - golden).abs().max().item())
