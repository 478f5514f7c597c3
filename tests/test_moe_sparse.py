"""Index-based ("sparse") MoE routing against the dense GShard path:
routing plans, dispatch/combine, gradients, the layer and 2-proc gloo
training. CPU-only; the kernels are covered by test_gpu_moe_kernels.py."""

import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests.internal.multi_process import run_multi_process

# (tokens, experts, capacity_factor)
CASES = [(1, 1, 1.0), (63, 4, 1.0), (257, 7, 0.5), (1000, 64, 1.0),
         (1000, 130, 2.0), (5000, 8, 0.25)]
MIN_CAPACITY = 4
F32_EPS = torch.finfo(torch.float32).eps


@functools.lru_cache(maxsize=None)
def _route(S, E, cf, k, masked=False):
    """Dense and sparse gate results for one case, from the same seed."""
    from bagua_amd.parallel.moe.sharded_moe import (
        top1gating, top1routing, top2gating, top2routing)

    torch.manual_seed(1000 + S + E)
    logits = torch.randn(S, E)
    used = (torch.rand(S) < 0.7).long() if masked else None
    if k == 1:
        torch.manual_seed(7)
        dense = top1gating(logits, cf, MIN_CAPACITY, used)
        torch.manual_seed(7)
        sparse = top1routing(logits, cf, MIN_CAPACITY, used)
    else:
        torch.manual_seed(7)
        dense = top2gating(logits, cf, MIN_CAPACITY)
        torch.manual_seed(7)
        sparse = top2routing(logits, cf, MIN_CAPACITY)
    return dense, sparse


def _scatter_plan(plan, S):
    """The (S, E, C) combine_weights a plan stands for."""
    E, C = plan.num_experts, plan.capacity
    cw = torch.zeros(S, E * C)
    for j in range(plan.dest.shape[0]):
        keep = plan.dest[j] >= 0
        tok = torch.arange(S)[keep]
        cw[tok, plan.dest[j][keep].long()] = plan.weights[j][keep]
    return cw.reshape(S, E, C)


def _check_plan_equals_dense(S, E, cf, k, masked=False):
    (l_aux_d, cw, mask, counts_d), (l_aux_s, plan, counts_s) = _route(
        S, E, cf, k, masked)
    assert plan.num_experts == E and plan.capacity == cw.shape[2]
    assert plan.dest.dtype == torch.int32 and plan.dest.shape == (k, S)
    assert plan.weights.dtype == torch.float32
    assert plan.src.dtype == torch.int32
    assert torch.equal(_scatter_plan(plan, S), cw)
    assert counts_s.dtype == torch.int64
    assert torch.equal(counts_s, counts_d)
    torch.testing.assert_close(l_aux_s, l_aux_d, rtol=1e-6, atol=0)


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("S,E,cf", CASES)
def test_plan_equals_dense(S, E, cf, k):
    _check_plan_equals_dense(S, E, cf, k)


def test_plan_equals_dense_used_token():
    _check_plan_equals_dense(257, 7, 0.5, 1, masked=True)
    (_, _, _, _), (_, plan, _) = _route(257, 7, 0.5, 1, True)
    torch.manual_seed(1000 + 257 + 7)
    torch.randn(257, 7)
    used = (torch.rand(257) < 0.7).long()
    assert 0 < int(used.sum()) < 257
    assert bool((plan.dest[0][used == 0] == -1).all())


def test_cases_cover_no_drop_and_heavy_drop():
    fractions = []
    for S, E, cf in CASES:
        for k in (1, 2):
            _, (_, plan, counts) = _route(S, E, cf, k)
            kept = int((plan.dest >= 0).sum())
            assert kept == int(counts.sum())
            fractions.append(1.0 - kept / (k * S))
    assert min(fractions) == 0.0, fractions
    assert max(fractions) > 0.5, fractions


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("S,E,cf", CASES)
def test_src_is_inverse_of_dest(S, E, cf, k):
    _, (_, plan, _) = _route(S, E, cf, k)
    tok = torch.arange(S, dtype=torch.int32).repeat(k, 1)
    keep = plan.dest >= 0
    rows = plan.dest[keep].long()
    assert rows.unique().numel() == rows.numel(), "a row is double-booked"
    assert torch.equal(plan.src[rows], tok[keep])
    others = torch.ones_like(plan.src, dtype=torch.bool)
    others[rows] = False
    assert bool((plan.src[others] == -1).all())
    assert plan.src.numel() == plan.num_experts * plan.capacity


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("S,E,cf", CASES)
def test_dispatch_combine_equal_dense_einsums(S, E, cf, k):
    from bagua_amd.ops import moe as moe_ops

    (_, cw, mask, _), (_, plan, _) = _route(S, E, cf, k)
    M = 61
    C = plan.capacity
    torch.manual_seed(3)
    x = torch.randn(S, M)
    eo = torch.randn(E, C, M)

    dense_disp = torch.einsum("sec,sm->ecm", mask.to(x.dtype), x)
    disp = moe_ops.dispatch(x, plan)
    assert disp.shape == (E * C, M)
    assert torch.equal(disp.reshape(E, C, M), dense_disp)

    comb = moe_ops.combine(eo.reshape(E * C, M), plan)
    assert comb.shape == (S, M)
    if k == 1:
        dense_comb = torch.einsum("sec,ecm->sm", cw, eo)
        assert torch.equal(comb, dense_comb)
    else:
        ref = torch.einsum("sec,ecm->sm", cw.double(), eo.double())
        mag = torch.einsum("sec,ecm->sm", cw.double(), eo.double().abs())
        bound = 4 * F32_EPS * mag + torch.finfo(torch.float32).tiny
        err = (comb.double() - ref).abs()
        assert bool((err <= bound).all()), float((err - bound).max())


def _small_plan(dtype=torch.float64):
    """S=12, E=3, C=3, k=2: 24 choices into 9 slots, most dropped."""
    from bagua_amd.ops import moe as moe_ops

    S, E, C = 12, 3, 3
    torch.manual_seed(11)
    e1 = torch.randint(0, E, (S,), dtype=torch.int32)
    e2 = (e1 + torch.randint(1, E, (S,), dtype=torch.int32)) % E
    s1, c1, src = moe_ops.assign_slots(e1, E, C)
    s2, c2, src = moe_ops.assign_slots(e2, E, C, base=c1, src=src)
    drop = torch.full_like(s1, -1)
    dest = torch.stack([torch.where(s1 < C, e1 * C + s1, drop),
                        torch.where(s2 < C, e2 * C + s2, drop)])
    assert int((dest >= 0).sum()) == E * C and int((dest < 0).sum()) > 0
    weights = torch.rand(2, S, dtype=dtype) + 0.1
    return moe_ops.RoutingPlan(dest, weights, src, E, C)


def test_gradcheck_dispatch():
    from bagua_amd.ops import moe as moe_ops

    plan = _small_plan()
    x = torch.randn(12, 5, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda t: moe_ops.dispatch(t, plan),
                                    (x,))


def test_gradcheck_combine():
    from bagua_amd.ops import moe as moe_ops

    plan = _small_plan()
    eo = torch.randn(9, 5, dtype=torch.float64, requires_grad=True)
    w = plan.weights.clone().requires_grad_(True)

    def fn(eo_, w_):
        return moe_ops.combine(eo_, plan._replace(weights=w_))

    assert torch.autograd.gradcheck(fn, (eo, w))


def _make_layer(routing, k, hidden=16, experts=4):
    from bagua_amd.parallel.moe import MoE

    torch.manual_seed(21)
    return MoE(hidden,
               expert=nn.Sequential(nn.Linear(hidden, 32), nn.ReLU(),
                                    nn.Linear(32, hidden)),
               num_local_experts=experts, k=k, routing=routing).double()


@pytest.mark.parametrize("k", [1, 2])
def test_layer_dense_equals_sparse_float64(k):
    torch.manual_seed(5)
    x0 = torch.randn(40, 16, dtype=torch.float64)
    proj = torch.randn(40, 16, dtype=torch.float64)
    results = {}
    for routing in ("dense", "sparse"):
        layer = _make_layer(routing, k)
        x = x0.clone().requires_grad_(True)
        torch.manual_seed(9)  # top-2 draws gumbel noise
        out, l_aux, counts = layer(x)
        ((out * proj).sum() + l_aux).backward()
        results[routing] = (out.detach(), x.grad, counts,
                            {n: p.grad for n, p in layer.named_parameters()})
    d, s = results["dense"], results["sparse"]
    assert int(d[2].sum()) < k * 40, "case drops nothing"
    assert torch.equal(d[2], s[2])
    torch.testing.assert_close(s[0], d[0], rtol=1e-10, atol=1e-12)
    torch.testing.assert_close(s[1], d[1], rtol=1e-10, atol=1e-12)
    assert d[3].keys() == s[3].keys()
    for name in d[3]:
        assert d[3][name] is not None and s[3][name] is not None, name
        torch.testing.assert_close(s[3][name], d[3][name], rtol=1e-10,
                                   atol=1e-12, msg=lambda m: name + ": " + m)


class MoEModel(nn.Module):
    """The small model of tests/test_moe.py with a routing switch."""

    def __init__(self, hidden=16, num_local_experts=2, k=1,
                 routing="dense"):
        super().__init__()
        from bagua_amd.parallel.moe import MoE

        self.fc1 = nn.Linear(8, hidden)
        self.moe = MoE(hidden,
                       expert=nn.Sequential(nn.Linear(hidden, 32),
                                            nn.ReLU(),
                                            nn.Linear(32, hidden)),
                       num_local_experts=num_local_experts, k=k,
                       routing=routing)
        self.out = nn.Linear(hidden, 4)

    def forward(self, x):
        x = F.relu(self.fc1(x))
        x, l_aux, _ = self.moe(x)
        return self.out(x), l_aux


def _worker_moe_train(rank, nprocs, k, routing):
    import bagua_amd
    from bagua_amd.parallel.algorithms.gradient_allreduce import (
        GradientAllReduceAlgorithm,
    )
    from bagua_amd.parallel.moe import is_moe_param

    bagua_amd.init_process_group()
    torch.manual_seed(13 + rank)
    model = MoEModel(k=k, routing=routing)
    optimizer = torch.optim.SGD(model.parameters(), lr=0.05)
    ddp = bagua_amd.DistributedDataParallel(
        model, optimizers=[optimizer],
        algorithm=GradientAllReduceAlgorithm())

    losses = []
    for step in range(8):
        torch.manual_seed(500 + rank * 31 + step)
        data = torch.randn(16, 8)
        target = torch.randn(16, 4)
        optimizer.zero_grad()
        out, l_aux = ddp(data)
        loss = F.mse_loss(out, target) + 0.01 * l_aux
        loss.backward()
        optimizer.step()
        losses.append(loss.item())

    dense = torch.cat([p.detach().reshape(-1)
                       for n, p in sorted(model.named_parameters())
                       if not is_moe_param(p)])
    expert = torch.cat([p.detach().reshape(-1)
                        for n, p in sorted(model.named_parameters())
                        if is_moe_param(p)])
    bagua_amd.deinit_process_group()
    return dense, expert, losses


@pytest.mark.parametrize("k", [1, 2])
def test_moe_train_sparse_matches_dense_2proc(k):
    runs = {routing: run_multi_process(2, _worker_moe_train,
                                       args=(k, routing))
            for routing in ("sparse", "dense")}
    for routing, out in runs.items():
        assert torch.equal(out[0][0], out[1][0]), (
            "%s: dense params diverged" % routing)
        assert not torch.equal(out[0][1], out[1][1]), (
            "%s: expert params identical across EP ranks" % routing)
    for rank in range(2):
        sparse = torch.tensor(runs["sparse"][rank][2])
        dense = torch.tensor(runs["dense"][rank][2])
        assert bool(torch.isfinite(sparse).all())
        torch.testing.assert_close(sparse, dense, rtol=1e-4, atol=0)


def test_unknown_routing_raises():
    from bagua_amd.parallel.moe import MoE, TopKGate

    with pytest.raises(ValueError):
        MoE(8, expert=nn.Linear(8, 8), routing="foo")
    with pytest.raises(ValueError):
        TopKGate(8, 4, routing="foo")


def test_sparse_without_drop_tokens_raises():
    from bagua_amd.parallel.moe import MoE, TopKGate

    with pytest.raises(ValueError):
        MoE(8, expert=nn.Linear(8, 8), routing="sparse", drop_tokens=False)
    with pytest.raises(ValueError):
        TopKGate(8, 4, routing="sparse", drop_tokens=False)
