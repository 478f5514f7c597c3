#!/usr/bin/env python3
"""Micro-benchmark MoE token routing: dense einsums vs index-based rows.

Times one ``MoE`` layer's forward plus backward on one GPU with
``routing="dense"`` and ``routing="sparse"``, for top-1 and top-2 gating
in f32 and bf16, and prints the peak memory of each. The expert FFN
(d_model -> 4*d_model -> d_model) is identical in both, so the difference
is the token movement around it.
"""

import argparse
import os
import sys
import time

import torch
import torch.nn as nn

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                "..", ".."))

from bagua_amd.ops import native
from bagua_amd.parallel.moe import MoE


def bench(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def run(routing, tokens, experts, d_model, k, dtype, iters, warmup):
    torch.manual_seed(0)
    with torch.device("cuda"):  # build the experts on the GPU directly
        layer = MoE(d_model,
                    expert=nn.Sequential(nn.Linear(d_model, 4 * d_model),
                                         nn.ReLU(),
                                         nn.Linear(4 * d_model, d_model)),
                    num_local_experts=experts, k=k,
                    routing=routing).to(dtype)
    x = torch.randn(tokens, d_model, device="cuda").to(dtype)
    x.requires_grad_(True)

    def step():
        layer.zero_grad(set_to_none=True)
        x.grad = None
        out, l_aux, _ = layer(x)
        (out.float().sum() + l_aux).backward()

    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    ms = bench(step, iters, warmup)
    return ms, torch.cuda.max_memory_allocated() / 2 ** 20


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--iters", type=int, default=10)
    parser.add_argument("--warmup", type=int, default=3)
    parser.add_argument("--d-model", type=int, default=1024)
    args = parser.parse_args()
    native.require()

    print("# " + " ".join(["python"] + sys.argv))
    print("# %s, one MoE layer forward+backward, d_model=%d, %d iters "
          "after %d warm-up" % (torch.cuda.get_device_name(0),
                                args.d_model, args.iters, args.warmup))
    print("%-6s %-3s %7s %7s %10s %10s %8s %11s %11s"
          % ("dtype", "k", "tokens", "experts", "dense ms", "sparse ms",
             "speedup", "dense MiB", "sparse MiB"))
    for dtype, name in [(torch.float32, "f32"), (torch.bfloat16, "bf16")]:
        for k in (1, 2):
            for tokens in (2048, 8192):
                for experts in (8, 64):
                    d_ms, d_mem = run("dense", tokens, experts,
                                      args.d_model, k, dtype, args.iters,
                                      args.warmup)
                    s_ms, s_mem = run("sparse", tokens, experts,
                                      args.d_model, k, dtype, args.iters,
                                      args.warmup)
                    print("%-6s %-3d %7d %7d %10.3f %10.3f %7.2fx %11.1f "
                          "%11.1f" % (name, k, tokens, experts, d_ms, s_ms,
                                      d_ms / s_ms, d_mem, s_mem),
                          flush=True)


if __name__ == "__main__":
    main()
