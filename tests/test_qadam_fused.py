"""FusedQAdamOptimizer on the CPU/gloo tier: the single-op bucket path
against the QAdam golden simulation, and the state round trip."""

import torch
import torch.nn.functional as F

from tests import test_qadam_golden as G
from tests.internal.multi_process import run_multi_process


def _worker(rank, nprocs):
    import bagua_amd
    from bagua_amd.parallel.algorithms.q_adam import (
        FusedQAdamOptimizer,
        QAdamAlgorithm,
    )

    bagua_amd.init_process_group()
    torch.manual_seed(13 + rank)
    model = G.TinyNet()
    optimizer = FusedQAdamOptimizer(model.parameters(), lr=G.LR,
                                    warmup_steps=G.WARMUP)
    ddp = bagua_amd.DistributedDataParallel(
        model, optimizers=[optimizer], algorithm=QAdamAlgorithm(optimizer))
    for step in range(G.STEPS):
        data, target = G._data(rank, step)
        optimizer.zero_grad()
        F.mse_loss(ddp(data), target).backward()
        optimizer.step()
    ops = [len(b.ops) for b in ddp.bagua_buckets]
    flat = torch.cat([p.detach().reshape(-1) for p in model.parameters()])
    bagua_amd.deinit_process_group()
    return flat, ops


def test_fused_qadam_matches_golden():
    nprocs = 2
    out = run_multi_process(nprocs, _worker)
    golden = G._simulate(nprocs)
    for rank in range(nprocs):
        flat, ops = out[rank]
        assert ops and all(n == 1 for n in ops), ops
        assert torch.allclose(flat, golden[rank], atol=1e-6), (
            "rank %d deviates from golden QAdam trajectory (max %g)"
            % (rank, (flat - golden[rank]).abs().max()))


def test_state_round_trip_keeps_views():
    from bagua_amd.parallel.algorithms.q_adam import FusedQAdamOptimizer

    def run(model, opt, steps):
        for step in steps:
            data, target = G._data(0, step)
            opt.zero_grad()
            F.mse_loss(model(data), target).backward()
            opt.step()

    torch.manual_seed(5)
    a = G.TinyNet()
    oa = FusedQAdamOptimizer(a.parameters(), lr=G.LR, warmup_steps=G.WARMUP)
    run(a, oa, range(G.WARMUP - 1))
    b = G.TinyNet()
    b.load_state_dict(a.state_dict())
    ob = FusedQAdamOptimizer(b.parameters(), lr=G.LR, warmup_steps=G.WARMUP)
    ob.load_state_dict(oa.state_dict())
    flat_v = ob._flat[0]["exp_avg_sq"]
    offset = 0
    for pa, pb in zip(a.parameters(), b.parameters()):
        sa, sb = oa.state[pa], ob.state[pb]
        assert sb["step"] == sa["step"] == G.WARMUP - 1
        assert sb["exp_avg_sq"].data_ptr() == flat_v.data_ptr() + 4 * offset
        assert torch.equal(sb["exp_avg_sq"], sa["exp_avg_sq"])
        assert torch.equal(sb["exp_avg"], sa["exp_avg"])
        offset += pb.numel()
    assert bool(flat_v.any())
    # across the boundary both take the same steps
    run(a, oa, range(G.WARMUP - 1, G.WARMUP + 2))
    run(b, ob, range(G.WARMUP - 1, G.WARMUP + 2))
    offset = 0
    for pa, pb in zip(a.parameters(), b.parameters()):
        assert torch.equal(pa, pb)
        assert ob.state[pb]["exp_avg_sq"].data_ptr() \
            == flat_v.data_ptr() + 4 * offset
        offset += pb.numel()
