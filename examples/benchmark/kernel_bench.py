#!/usr/bin/env python3
"""Micro-benchmark the CDNA4 kernel pack vs the HBM3E roofline.

Every kernel is memory-bound; the table prints achieved GB/s next to the
theoretical bytes moved. MI355X HBM3E peak is 8 TB/s (≈6.3 achievable).
"""

import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                "..", ".."))

from bagua_amd.ops import native


def bench(fn, bytes_moved, iters=50, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / iters
    return bytes_moved / dt / 1e9, dt * 1e6


def sync_batchnorm_rows():
    """SyncBatchNorm's kernels at ResNet-50's BN shapes (bf16 channels-last,
    batch 32) and VGG-bn's first (f32 NCHW, batch 8), each next to the torch
    chain it replaces on the same tensors. Bytes are the passes the
    algorithm needs in the input's dtype: stats reads x, apply reads x and
    writes y (3 passes forward), bwd_reduce reads dy and x, bwd_apply reads
    dy and x and writes dx (5 backward); the chain's rows count the same
    bytes."""
    from bagua_amd.contrib import sync_batchnorm
    from bagua_amd.ops import batchnorm as bn_ops

    rows = []
    shapes = [(torch.bfloat16, True, (32, 64, 112, 112)),
              (torch.bfloat16, True, (32, 256, 56, 56)),
              (torch.bfloat16, True, (32, 512, 28, 28)),
              (torch.bfloat16, True, (32, 2048, 7, 7)),
              (torch.float32, False, (8, 64, 224, 224))]
    for dtype, cl, shape in shapes:
        c = shape[1]
        name = "bf16" if dtype == torch.bfloat16 else "f32"
        tag = "@%dx%dx%d%s" % (c, shape[2], shape[3], "cl" if cl else "")
        fmt = torch.channels_last if cl else torch.contiguous_format
        x = torch.randn(shape, device="cuda").to(dtype).contiguous(
            memory_format=fmt)
        dy = torch.randn_like(x)
        w = torch.rand(c, device="cuda") + 0.5
        b = torch.randn(c, device="cuda")
        rm, rv = torch.zeros(c, device="cuda"), torch.ones(c, device="cuda")
        nbytes = x.numel() * x.element_size()
        assert bn_ops.kernels_apply(x, w, b, rm, rv, 0.1)
        stats = bn_ops.stats(x)
        _, mi = bn_ops.apply(x, stats, w, b, rm, rv, 0.1, 1e-5)
        packed, _, _ = bn_ops.backward_reduce(dy, x, mi, w, b)

        # the module's function both ways, kernels and the torch chain
        # they replace, alternating, twice for the spread; no allreduce in
        # either (a world of one rank)
        fn = sync_batchnorm._SyncBatchNormFn
        leaves = [t.clone().requires_grad_() for t in (x, w, b)]

        def forward():
            with torch.no_grad():
                return fn.apply(x, w, b, rm, rv, 1e-5, 0.1)

        def both():
            y = fn.apply(*leaves, rm, rv, 1e-5, 0.1)
            return torch.autograd.grad(y, leaves, dy)

        saved = (bn_ops.kernels_apply, sync_batchnorm.allreduce_inplace)
        sync_batchnorm.allreduce_inplace = lambda t, op=None: None
        try:
            for _ in range(2):
                for label, call, passes in (("fwd", forward, 3),
                                            ("fwd+bwd", both, 8)):
                    bn_ops.kernels_apply = saved[0]
                    gbs, us = bench(call, passes * nbytes)
                    rows.append(("bn_" + label + tag, name, gbs, us))
                    bn_ops.kernels_apply = lambda *a, **k: False
                    gbs, us = bench(call, passes * nbytes)
                    rows.append(("  torch chain " + label, name, gbs, us))
        finally:
            bn_ops.kernels_apply, sync_batchnorm.allreduce_inplace = saved
        for label, call, passes in (
                ("bn_stats", lambda: bn_ops.stats(x), 1),
                ("bn_apply", lambda: bn_ops.apply(
                    x, stats, w, b, rm, rv, 0.1, 1e-5), 2),
                ("bn_bwd_reduce", lambda: bn_ops.backward_reduce(
                    dy, x, mi, w, b), 2),
                ("bn_bwd_apply", lambda: bn_ops.backward_apply(
                    dy, x, packed, stats, mi, w), 3)):
            gbs, us = bench(call, passes * nbytes)
            rows.append((label + tag, name, gbs, us))
    return rows


def sync_batchnorm_act_rows():
    """relu(bn(x)) and relu(bn(x) + z), forward and backward, at ResNet-50's
    BN shapes (bf16 channels-last, batch 32): the fused function next to
    the unfused composition through ``_SyncBatchNormFn`` and torch's add
    and relu, alternating, twice for the spread; no allreduce in either.
    Bytes are the fused path's passes in the input's dtype with the sign
    mask a sixteenth of one: ReLU 3 1/16 forward and 5 1/8 backward,
    add+ReLU one more each way (read z, write dz); the unfused rows count
    the same bytes (they move 13 and 16 passes)."""
    from bagua_amd.contrib import sync_batchnorm
    from bagua_amd.ops import batchnorm as bn_ops

    rows = []
    saved = sync_batchnorm.allreduce_inplace
    sync_batchnorm.allreduce_inplace = lambda t, op=None: None
    try:
        for shape in ((32, 64, 112, 112), (32, 256, 56, 56),
                      (32, 512, 28, 28), (32, 2048, 7, 7)):
            c = shape[1]
            tag = "@%dx%dx%dcl" % (c, shape[2], shape[3])
            x = torch.randn(shape, device="cuda").to(
                torch.bfloat16).contiguous(memory_format=torch.channels_last)
            dy, z = torch.randn_like(x), torch.randn_like(x)
            w = torch.rand(c, device="cuda") + 0.5
            b = torch.randn(c, device="cuda")
            rm = torch.zeros(c, device="cuda")
            rv = torch.ones(c, device="cuda")
            nbytes = x.numel() * x.element_size()
            assert bn_ops.kernels_apply(x, w, b, rm, rv, 0.1)
            for label, res, passes in (("relu", None, 8.1875),
                                       ("add_relu", z, 10.1875)):
                leaves = [t.clone().requires_grad_()
                          for t in (x, w, b) + (() if res is None else (z,))]

                def fused():
                    y = sync_batchnorm._SyncBatchNormActFn.apply(
                        leaves[0], leaves[3] if res is not None else None,
                        leaves[1], leaves[2], rm, rv, 1e-5, 0.1)
                    return torch.autograd.grad(y, leaves, dy)

                def unfused():
                    y = sync_batchnorm._SyncBatchNormFn.apply(
                        leaves[0], leaves[1], leaves[2], rm, rv, 1e-5, 0.1)
                    if res is not None:
                        y = y + leaves[3]
                    return torch.autograd.grad(torch.relu(y), leaves, dy)

                for _ in range(2):
                    gbs, us = bench(fused, passes * nbytes)
                    rows.append(("bn_%s fwd+bwd%s" % (label, tag), "bf16",
                                 gbs, us))
                    gbs, us = bench(unfused, passes * nbytes)
                    rows.append(("  unfused bn, %s" % label, "bf16", gbs,
                                 us))
    finally:
        sync_batchnorm.allreduce_inplace = saved
    return rows


def conv_epilogue_pool_rows():
    """The pooled conv epilogue at VGG16's largest pooled stage, 32 x 64 x
    224 x 224 bf16 channels-last, each kernel alone: the pair that keeps y
    and the compact pair next to it. Bytes with y the conv output (2 B an
    element), p and g a quarter of it and the code half of p: keeping y,
    forward reads and writes y and writes p, backward reads g and y and
    writes dx; compact, forward reads the conv output and writes p and the
    code, backward reads g and the code and writes dx."""
    lib = native.require()
    cl = dict(memory_format=torch.channels_last)
    x = torch.randn(32, 64, 224, 224, device="cuda",
                    dtype=torch.bfloat16).contiguous(**cl)
    b = torch.randn(64, device="cuda", dtype=torch.bfloat16)
    p = torch.empty(32, 64, 112, 112, device="cuda",
                    dtype=torch.bfloat16).contiguous(**cl)
    g = torch.randn_like(p)
    code = torch.empty(32, 112, 112, 64, device="cuda", dtype=torch.uint8)
    dx = torch.empty_like(x)
    db = torch.empty_like(b)
    yb, pb, cb = 2 * x.numel(), 2 * p.numel(), code.numel()
    lib.conv_bias_relu_pool_code(x, b, p, code)
    rows = []
    for _ in range(2):  # twice for the spread
        for label, call, nbytes in (
                ("epi_pool_code_fwd",
                 lambda: lib.conv_bias_relu_pool_code(x, b, p, code),
                 yb + pb + cb),
                ("epi_pool_code_bwd",
                 lambda: lib.conv_pool_code_bwd(g, code, dx, db),
                 pb + cb + yb),
                # in place: x is relu'd again and again, same work each time
                ("epi_pool_fwd (keeps y)",
                 lambda: lib.conv_bias_relu_pool_(x, b, p), 2 * yb + pb),
                ("epi_pool_bwd (reads y)",
                 lambda: lib.conv_pool_relu_bwd(g, x, dx, db),
                 pb + 2 * yb)):
            gbs, us = bench(call, nbytes)
            rows.append((label + "@vgg", "bf16", gbs, us))
    return rows


def main():
    lib = native.require()
    n = 1 << 26  # 64 Mi elements
    results = []

    for dtype, name in [(torch.float32, "f32"), (torch.float16, "f16"),
                        (torch.bfloat16, "bf16")]:
        es = torch.tensor([], dtype=dtype).element_size()
        x = torch.randn(n, device="cuda").to(dtype)
        y = torch.randn(n, device="cuda").to(dtype)

        gbs, us = bench(lambda: lib.average_inplace(x, y), 3 * n * es)
        results.append(("average_inplace", name, gbs, us))

        gbs, us = bench(lambda: lib.addmul_inplace(x, y, 0.3), 3 * n * es)
        results.append(("addmul_inplace", name, gbs, us))

        chunks = 8
        gbs, us = bench(
            lambda: lib.reduce_chunk_inplace(x, chunks, 0, True),
            n * es + (n // chunks) * es)
        results.append(("reduce_chunk(8)", name, gbs, us))

        chunk = n // chunks
        stride = lib.compressed_chunk_stride(chunk)
        wire = torch.empty(stride * chunks, dtype=torch.uint8,
                           device="cuda")
        # compress = minmax read (n*es) + quantize read (n*es) + write n
        gbs, us = bench(lambda: lib.compress_chunked(x, wire, chunks, -1),
                        2 * n * es + n)
        results.append(("compress_chunked", name, gbs, us))

        gbs, us = bench(
            lambda: lib.decompress_chunked(wire, x, chunks, -1),
            n + n * es)
        results.append(("decompress_chunked", name, gbs, us))

        # fused dequantize+reduce (ByteGrad hot path) vs the unfused
        # chain it replaces: decompress (n + n*es) + reduce
        # (n*es + chunk*es) -> fused reads n u8 + writes chunk*es only
        gbs, us = bench(
            lambda: lib.dequant_reduce(wire, x, chunks, 0, True),
            n + chunk * es)
        results.append(("dequant_reduce(8)", name, gbs, us))

        def unfused():
            lib.decompress_chunked(wire, x, chunks, -1)
            lib.reduce_chunk_inplace(x, chunks, 0, True)

        gbs, us = bench(unfused, n + chunk * es)  # same useful bytes
        results.append(("  unfused chain", name, gbs, us))

    m = torch.zeros(n, device="cuda")
    g = torch.randn(n, device="cuda")
    p = torch.randn(n, device="cuda")
    v = torch.zeros(n, device="cuda")
    gbs, us = bench(lambda: lib.fused_sgd_step(
        p, g, m, 0.01, 0.9, 0.0, 1e-4, False, True), 5 * n * 4)
    results.append(("fused_sgd_step", "f32", gbs, us))
    gbs, us = bench(lambda: lib.fused_adam_step(
        p, g, m, v, 10, 1e-3, 0.9, 0.999, 1e-8, 0.0, False), 7 * n * 4)
    results.append(("fused_adam_step", "f32", gbs, us))

    # pure-bf16 flagship path: bf16 params/grads + fp32 master & momentum
    pb = torch.randn(n, device="cuda", dtype=torch.bfloat16)
    gb = torch.randn(n, device="cuda", dtype=torch.bfloat16)
    master = pb.float()
    mm = torch.zeros(n, device="cuda")
    # bytes: read g (2B) + master (4) + m (4); write p (2) + master (4) + m (4)
    gbs, us = bench(lambda: lib.fused_sgd_mixed_step(
        pb, gb, master, mm, 0.01, 0.9, 0.0, 1e-4, False, True), 20 * n)
    results.append(("fused_sgd_mixed", "bf16", gbs, us))
    del pb, gb, master, mm

    # the same step at VGG16's size, flat and through the segmented entry
    # point with VGG16's 32 gradient tensors, each its own allocation as
    # autograd leaves them. Same 20 B per parameter either way.
    from bagua_amd.models import vgg16

    with torch.device("meta"):
        numels = [q.numel() for q in vgg16(num_classes=1000).parameters()]
    offsets = [0]
    for k in numels:
        offsets.append(offsets[-1] + k)
    nv = offsets[-1]
    pb = torch.randn(nv, device="cuda", dtype=torch.bfloat16)
    gb = torch.randn(nv, device="cuda", dtype=torch.bfloat16)
    master = pb.float()
    mm = torch.zeros(nv, device="cuda")
    gbs, us = bench(lambda: lib.fused_sgd_mixed_step(
        pb, gb, master, mm, 0.01, 0.9, 0.0, 1e-4, False, True), 20 * nv)
    results.append(("fused_sgd_mixed@vgg", "bf16", gbs, us))
    grads = [gb[a:b].clone() for a, b in zip(offsets, offsets[1:])]
    gbs, us = bench(lambda: lib.fused_sgd_mixed_step_segments(
        pb, grads, offsets, master, mm, 0.01, 0.9, 0.0, 1e-4, False, True),
        20 * nv)
    results.append(("fused_sgd_mixed_segments", "bf16", gbs, us))

    del pb, gb, master, mm, grads

    # QAdam after warmup at VGG16's size, one bucket of 8 chunks, the 32
    # gradients (momenta) each their own allocation. Momentum + wire: read
    # m and g, write m (12 B), quantize reads m and writes u8 (5 B); the
    # unfused pair next to it is minmax + quantize alone (4 + 5 B, it has
    # no update). Frozen step: read w, v and m, write w (16 B); fused Adam
    # on the same tensors for scale (28 B).
    chunks = 8
    nm = (nv + 32 * chunks - 1) // (32 * chunks) * (32 * chunks)
    fm = torch.randn(nm, device="cuda") * 0.1
    gq = [torch.randn(b - a, device="cuda")
          for a, b in zip(offsets, offsets[1:])]
    wire = torch.empty(lib.compressed_chunk_stride(nm // chunks) * chunks,
                       dtype=torch.uint8, device="cuda")
    gbs, us = bench(lambda: lib.qadam_momentum_compress_chunked(
        fm, gq, offsets, 0.9, wire, chunks), 17 * nm)
    results.append(("qadam_momentum_compress@vgg", "f32", gbs, us))
    gbs, us = bench(lambda: lib.compress_chunked(fm, wire, chunks, -1),
                    9 * nm)
    results.append(("  minmax + quantize@vgg", "f32", gbs, us))
    fw = torch.randn(nv, device="cuda")
    fv = torch.rand(nv, device="cuda")
    gbs, us = bench(lambda: lib.qadam_frozen_step_segments(
        fw, gq, offsets, fv, 200, 1e-3, 0.9, 0.999, 1e-8), 16 * nv)
    results.append(("qadam_frozen_step@vgg", "f32", gbs, us))
    fmm = torch.zeros(nv, device="cuda")
    gbs, us = bench(lambda: lib.fused_adam_step_segments(
        fw, gq, offsets, fmm, fv, 200, 1e-3, 0.9, 0.999, 1e-8, 0.0, False),
        28 * nv)
    results.append(("  fused_adam_segments@vgg", "f32", gbs, us))
    del fm, gq, wire, fw, fv, fmm

    # VGG16's first stage at the flagship's size, 32 x 224 x 224:
    # Conv2d(3, 64, 3, padding=1) + bias + ReLU as one kernel each way.
    # bytes: forward reads x and writes y; backward reads g, y and x
    # (weights, bias and the f32 partial sums are noise next to those)
    cl = dict(memory_format=torch.channels_last)
    xi = torch.randn(32, 3, 224, 224, device="cuda",
                     dtype=torch.bfloat16).contiguous(**cl)
    wt = torch.randn(64, 3, 3, 3, device="cuda", dtype=torch.bfloat16) * 0.2
    bs = torch.randn(64, device="cuda", dtype=torch.bfloat16)
    yo = lib.first_conv_bias_relu(xi, wt, bs)
    go = torch.randn_like(yo)
    es = 2
    gbs, us = bench(lambda: lib.first_conv_bias_relu(xi, wt, bs),
                    (xi.numel() + yo.numel()) * es)
    results.append(("first_conv_fwd@vgg", "bf16", gbs, us))
    gbs, us = bench(lambda: lib.first_conv_bias_relu_bwd(go, yo, xi, wt),
                    (2 * yo.numel() + xi.numel()) * es)
    results.append(("first_conv_bwd@vgg", "bf16", gbs, us))

    del xi, wt, bs, yo, go
    results.extend(conv_epilogue_pool_rows())
    results.extend(sync_batchnorm_rows())
    results.extend(sync_batchnorm_act_rows())

    print("%-24s %-5s %10s %10s" % ("kernel", "dtype", "GB/s", "us"))
    for name, dt, gbs, us in results:
        print("%-24s %-5s %10.0f %10.1f" % (name, dt, gbs, us))


if __name__ == "__main__":
    main()
