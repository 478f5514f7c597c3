"""gfx950 MoE routing kernels (csrc/moe_kernels.hip) against the CPU torch
implementation of bagua_amd/ops/moe.py and the dense GShard path.
GPU-only."""

import functools

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

F32_EPS = torch.finfo(torch.float32).eps


# ---------------------------------------------------------------------------
# assign_slots
# ---------------------------------------------------------------------------

def _expert_draws(S, E, gen):
    uniform = torch.randint(0, E, (S,), generator=gen, dtype=torch.int32)
    skewed = torch.where(torch.rand(S, generator=gen) < 0.9,
                         torch.zeros_like(uniform), uniform)
    holes = torch.where(torch.rand(S, generator=gen) < 0.3,
                        torch.full_like(uniform, -1), uniform)
    single = torch.full((S,), E - 1, dtype=torch.int32)
    return {"uniform": uniform, "skewed": skewed, "holes": holes,
            "single": single}


@requires_gpu
@pytest.mark.parametrize("E", [1, 7, 64, 130, 1024])
@pytest.mark.parametrize("S", [1, 63, 64, 65, 257, 1000, 5000])
def test_assign_slots(S, E):
    from bagua_amd.ops import moe as moe_ops

    gen = torch.Generator().manual_seed(S * 4099 + E)
    base = torch.randint(0, 50, (E,), generator=gen, dtype=torch.int32)
    for name, expert in _expert_draws(S, E, gen).items():
        for capacity in (1, S):
            for b in (None, base):
                ref = moe_ops.assign_slots(expert, E, capacity, b)
                got = moe_ops.assign_slots(
                    expert.cuda(), E, capacity,
                    None if b is None else b.cuda())
                again = moe_ops.assign_slots(
                    expert.cuda(), E, capacity,
                    None if b is None else b.cuda())
                what = "%s capacity=%d base=%s" % (name, capacity,
                                                   b is not None)
                for r, g, a, field in zip(ref, got, again,
                                          ("slot", "counts", "src")):
                    assert g.dtype == torch.int32 and g.is_cuda
                    assert torch.equal(g.cpu(), r), "%s: %s" % (what, field)
                    assert torch.equal(g, a), "%s: %s rerun" % (what, field)


@requires_gpu
def test_assign_slots_continues_src():
    """top-2 use: the second call starts at the first call's counts and
    fills the same src."""
    from bagua_amd.ops import moe as moe_ops

    gen = torch.Generator().manual_seed(5)
    S, E, C = 1000, 7, 200
    e1 = torch.randint(0, E, (S,), generator=gen, dtype=torch.int32)
    e2 = (e1 + torch.randint(1, E, (S,), generator=gen,
                             dtype=torch.int32)) % E
    _, c1, src = moe_ops.assign_slots(e1, E, C)
    ref = moe_ops.assign_slots(e2, E, C, base=c1, src=src)
    _, g1, gsrc = moe_ops.assign_slots(e1.cuda(), E, C)
    got = moe_ops.assign_slots(e2.cuda(), E, C, base=g1, src=gsrc)
    for r, g in zip(ref, got):
        assert torch.equal(g.cpu(), r)


# ---------------------------------------------------------------------------
# row kernels
# ---------------------------------------------------------------------------

ROW_S, ROW_E = 257, 7


@functools.lru_cache(maxsize=None)
def _row_plan(k):
    """CPU plan for S=257, E=7 that drops about half of the choices."""
    from bagua_amd.ops import moe as moe_ops

    S, E = ROW_S, ROW_E
    C = 18 if k == 1 else 37
    gen = torch.Generator().manual_seed(40 + k)
    e1 = torch.randint(0, E, (S,), generator=gen, dtype=torch.int32)
    s1, c1, src = moe_ops.assign_slots(e1, E, C)
    drop = torch.full_like(s1, -1)
    dest = [torch.where(s1 < C, e1 * C + s1, drop)]
    if k == 2:
        e2 = (e1 + torch.randint(1, E, (S,), generator=gen,
                                 dtype=torch.int32)) % E
        s2, _, src = moe_ops.assign_slots(e2, E, C, base=c1, src=src)
        dest.append(torch.where(s2 < C, e2 * C + s2, drop))
    dest = torch.stack(dest)
    dropped = float((dest < 0).sum()) / dest.numel()
    assert 0.3 < dropped < 0.7, dropped
    # weights are random for dropped choices too: kernels must ignore them
    weights = torch.randn(k, S, generator=gen)
    return moe_ops.RoutingPlan(dest, weights, src, E, C)


def _rows(n, M, dtype, gen, misaligned):
    """(n, M) rows on the GPU; `misaligned` starts them one element into
    a larger buffer, so the base is not 16-byte aligned."""
    data = torch.randn(n, M, generator=gen).to(dtype)
    if not misaligned:
        return data.cuda()
    buf = torch.empty(n * M + 1, dtype=dtype, device="cuda")
    view = buf[1:].view(n, M)
    view.copy_(data)
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    return view


def _row_weight(plan):
    """float64 weight of the choice that fills each row, 0 if empty."""
    wr = torch.zeros(plan.src.numel(), dtype=torch.float64)
    for j in range(plan.dest.shape[0]):
        keep = plan.dest[j] >= 0
        wr[plan.dest[j][keep].long()] = plan.weights[j][keep].double()
    return wr


def _check_rows(k, M, dtype, misaligned=False):
    from bagua_amd.ops import moe as moe_ops

    plan = _row_plan(k)
    S, R = ROW_S, plan.src.numel()
    gen = torch.Generator().manual_seed(M * 31 + k)
    x = _rows(S, M, dtype, gen, misaligned)
    eo = _rows(R, M, dtype, gen, misaligned)
    src, dest, w = plan.src.cuda(), plan.dest.cuda(), plan.weights.cuda()
    eps_out = 0.0 if dtype == torch.float32 else torch.finfo(dtype).eps
    tiny = torch.finfo(dtype).tiny
    x64, eo64 = x.cpu().double(), eo.cpu().double()
    live = (plan.src >= 0).unsqueeze(1)
    sel = plan.src.long().clamp(min=0)

    def close(got, ref, mag, what):
        err = (got.cpu().double() - ref).abs()
        bound = (eps_out + 4 * F32_EPS) * mag + tiny
        assert bool((err <= bound).all()), "%s: worst excess %g" % (
            what, float((err - bound).max()))

    # gather without scale (dispatch forward): bitwise
    ref = moe_ops.gather_rows(x.cpu(), plan.src)
    got = moe_ops.gather_rows(x, src)
    assert got.dtype == dtype and got.shape == (R, M)
    assert torch.equal(got.cpu(), ref)
    assert torch.equal(got, moe_ops.gather_rows(x, src))

    # gather with scale (combine backward w.r.t. the expert output)
    ref = torch.where(live, _row_weight(plan).unsqueeze(1) * x64[sel],
                      torch.zeros(R, M, dtype=torch.float64))
    got = moe_ops.gather_rows(x, src, w, dest)
    close(got, ref, ref.abs(), "scaled gather")
    assert torch.equal(got, moe_ops.gather_rows(x, src, w, dest))

    # combine with and without weights
    for weights in (w, None):
        ref = torch.zeros(S, M, dtype=torch.float64)
        mag = torch.zeros(S, M, dtype=torch.float64)
        for j in range(k):
            wj = (plan.weights[j].double() if weights is not None
                  else torch.ones(S, dtype=torch.float64))
            term = wj.unsqueeze(1) * eo64[plan.dest[j].long().clamp(min=0)]
            term = torch.where((plan.dest[j] >= 0).unsqueeze(1), term,
                               torch.zeros_like(term))
            ref += term
            mag += term.abs()
        got = moe_ops.combine_rows(eo, dest, weights)
        assert got.dtype == dtype and got.shape == (S, M)
        close(got, ref, mag, "combine weights=%s" % (weights is not None))
        assert torch.equal(got, moe_ops.combine_rows(eo, dest, weights))

    # row dot (combine backward w.r.t. the weights)
    got = moe_ops.row_dot(x, eo, dest)
    assert got.dtype == torch.float32 and got.shape == (k, S)
    for j in range(k):
        prod = x64 * eo64[plan.dest[j].long().clamp(min=0)]
        keep = (plan.dest[j] >= 0).double()
        err = (got[j].cpu().double() - prod.sum(1) * keep).abs()
        bound = M * F32_EPS * prod.abs().sum(1) * keep
        assert bool((err <= bound).all()), "row_dot j=%d: excess %g" % (
            j, float((err - bound).max()))
    assert torch.equal(got, moe_ops.row_dot(x, eo, dest))


@requires_gpu
@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16,
                                   torch.bfloat16])
@pytest.mark.parametrize("M", [1, 8, 61, 64, 520])
def test_row_kernels(M, dtype, k):
    _check_rows(k, M, dtype)


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_row_kernels_misaligned_base(dtype):
    """M*elemsize is a multiple of 16 but the bases are not aligned: the
    launcher must pick the scalar path."""
    _check_rows(2, 64, dtype, misaligned=True)


@requires_gpu
def test_autograd_functions_on_gpu():
    """dispatch/combine backward on the GPU equal the CPU implementation
    run on the same f32 data (k=2, M=61)."""
    from bagua_amd.ops import moe as moe_ops

    plan = _row_plan(2)
    gen = torch.Generator().manual_seed(77)
    x = torch.randn(ROW_S, 61, generator=gen)
    eo = torch.randn(plan.src.numel(), 61, generator=gen)
    grads = {}
    for dev in ("cpu", "cuda"):
        def leaf(t):  # a fresh leaf: .to("cpu") alone would alias t
            return t.clone().to(dev).requires_grad_(True)

        p = moe_ops.RoutingPlan(plan.dest.to(dev), leaf(plan.weights),
                                plan.src.to(dev), plan.num_experts,
                                plan.capacity)
        xd, eod = leaf(x), leaf(eo)
        loss = moe_ops.dispatch(xd, p).pow(2).sum() \
            + moe_ops.combine(eod, p).pow(2).sum()
        loss.backward()
        grads[dev] = [t.grad.cpu() for t in (xd, eod, p.weights)]
    for c, g in zip(grads["cpu"], grads["cuda"]):
        torch.testing.assert_close(g, c, rtol=1e-5, atol=1e-5)


# ---------------------------------------------------------------------------
# layer
# ---------------------------------------------------------------------------

TOKENS, D_MODEL, EXPERTS = 300, 64, 4


def _make_layer(routing, k):
    from bagua_amd.parallel.moe import MoE

    torch.manual_seed(21)
    return MoE(D_MODEL,
               expert=nn.Sequential(nn.Linear(D_MODEL, 128), nn.ReLU(),
                                    nn.Linear(128, D_MODEL)),
               num_local_experts=EXPERTS, k=k, routing=routing)


def _run_layer(layer, x0, proj):
    x = x0.clone().requires_grad_(True)
    out, l_aux, counts = layer(x)
    ((out * proj).sum() + l_aux).backward()
    res = {"output": out.detach(), "input.grad": x.grad}
    for n, p in layer.named_parameters():
        res[n + ".grad"] = p.grad
    return {n: t.detach().cpu().double() for n, t in res.items()}, \
        counts.cpu()


@requires_gpu
@pytest.mark.parametrize("k", [1, 2])
def test_layer_sparse_vs_dense_f32(k, monkeypatch):
    from bagua_amd.parallel.moe import sharded_moe

    # one noise draw for every run: CPU and GPU generators differ
    noise = torch.distributions.gumbel.Gumbel(0.0, 1.0).sample(
        (TOKENS, EXPERTS))
    monkeypatch.setattr(sharded_moe, "gumbel_rsample",
                        lambda shape, device: noise.to(device))

    torch.manual_seed(5)
    x0 = torch.randn(TOKENS, D_MODEL)
    proj = torch.randn(TOKENS, D_MODEL)

    ref, ref_counts = _run_layer(_make_layer("dense", k).double(),
                                 x0.double(), proj.double())
    dense, dense_counts = _run_layer(_make_layer("dense", k).cuda(),
                                     x0.cuda(), proj.cuda())
    sparse, sparse_counts = _run_layer(_make_layer("sparse", k).cuda(),
                                       x0.cuda(), proj.cuda())
    assert torch.equal(sparse_counts, dense_counts)
    assert int(sparse_counts.sum()) < k * TOKENS, "case drops nothing"
    assert ref.keys() == dense.keys() == sparse.keys()
    for name in ref:
        err_dense = float((dense[name] - ref[name]).abs().max())
        err_sparse = float((sparse[name] - ref[name]).abs().max())
        floor = 64 * F32_EPS * float(ref[name].abs().max())
        print("k=%d %-40s dense_err=%.3e sparse_err=%.3e floor=%.3e"
              % (k, name, err_dense, err_sparse, floor))
        assert err_sparse <= max(4 * err_dense, floor), name


@requires_gpu
@pytest.mark.parametrize("k", [1, 2])
def test_layer_bf16_finite(k, monkeypatch):
    from bagua_amd.parallel.moe import sharded_moe

    noise = torch.distributions.gumbel.Gumbel(0.0, 1.0).sample(
        (TOKENS, EXPERTS)).cuda()
    monkeypatch.setattr(sharded_moe, "gumbel_rsample",
                        lambda shape, device: noise)
    torch.manual_seed(5)
    x0 = torch.randn(TOKENS, D_MODEL).cuda().bfloat16()
    proj = torch.randn(TOKENS, D_MODEL).cuda().bfloat16()
    dense, dense_counts = _run_layer(
        _make_layer("dense", k).cuda().bfloat16(), x0, proj)
    sparse, sparse_counts = _run_layer(
        _make_layer("sparse", k).cuda().bfloat16(), x0, proj)
    assert torch.equal(sparse_counts, dense_counts)
    for name, t in sparse.items():
        assert bool(torch.isfinite(t).all()), name


def _peak_memory(routing):
    from bagua_amd.parallel.moe import MoE

    torch.manual_seed(3)
    layer = MoE(64, expert=nn.Sequential(nn.Linear(64, 128), nn.ReLU(),
                                         nn.Linear(128, 64)),
                num_local_experts=8, k=1, routing=routing).cuda()
    x = torch.randn(4096, 64, device="cuda", requires_grad=True)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    out, l_aux, _ = layer(x)
    (out.sum() + l_aux).backward()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated()


@requires_gpu
def test_sparse_peak_memory_below_dense():
    dense = _peak_memory("dense")
    sparse = _peak_memory("sparse")
    print("peak memory: dense %.1f MiB, sparse %.1f MiB"
          % (dense / 2 ** 20, sparse / 2 ** 20))
    assert sparse < dense
