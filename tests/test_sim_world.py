"""The bucket sync protocols of bagua_amd/executor.py at world sizes 2, 3
and 8 in a simulated world (tests/internal/sim_world.py), on the CPU: the
torch paths of ``ops`` against the float64 derivations. The same cases run
on the GPU in tests/test_gpu_sim_world.py; passing here on the same inputs
shows that the reference alone meets every bound.

The last tests plant faults in ``bagua_amd.executor.ops`` and require the
cases to notice."""

import pytest
import torch

from tests.internal import sim_world as sw

DEVICE = "cpu"

grid = pytest.mark.parametrize(
    "n,dtype,chunk",
    [(n, d, c) for n in sw.WORLDS for d in sw.DTYPES for c in sw.CHUNKS],
    ids=lambda v: sw._name(v) if isinstance(v, torch.dtype) else str(v))
even_grid = pytest.mark.parametrize(
    "n,dtype,chunk",
    [(n, d, c) for n in (2, 8) for d in sw.DTYPES for c in sw.CHUNKS],
    ids=lambda v: sw._name(v) if isinstance(v, torch.dtype) else str(v))
averages = pytest.mark.parametrize("average", [True, False],
                                   ids=["avg", "sum"])


@grid
@averages
def test_scattergather_exact(n, dtype, chunk, average):
    sw.case_scattergather_exact(DEVICE, n, dtype, chunk, average)


@grid
@averages
def test_scattergather_random(n, dtype, chunk, average):
    sw.case_scattergather_random(DEVICE, n, dtype, chunk, average)


@grid
def test_bytegrad_exact(n, dtype, chunk):
    sw.case_bytegrad_exact(DEVICE, n, dtype, chunk)


@grid
@averages
def test_bytegrad_random(n, dtype, chunk, average):
    sw.case_bytegrad_random(DEVICE, n, dtype, chunk, average)


@even_grid
@pytest.mark.parametrize("exact", [False, True], ids=["random", "exact"])
def test_shift_one(n, dtype, chunk, exact):
    sw.case_shift_one(DEVICE, n, dtype, chunk, exact)


@grid
def test_low_prec_ring(n, dtype, chunk):
    sw.case_low_prec_ring(DEVICE, n, dtype, chunk)


# ---------------------------------------------------------------------------
# the harness itself
# ---------------------------------------------------------------------------

def test_collectives_move_the_right_chunks():
    n, chunk = 3, 5
    flats = [torch.arange(n * chunk, dtype=torch.float32) + 100 * r
             for r in range(n)]

    def a2a(comm, group, flat):
        t = flat.clone()
        comm.alltoall_inplace(t)
        return t

    def ag(comm, group, flat):
        t = flat.clone()
        comm.allgather_inplace(t)
        return t

    for r, t in enumerate(sw.run_world(n, a2a, flats)):
        for p in range(n):
            assert torch.equal(t.view(n, -1)[p], flats[p].view(n, -1)[r])
    for r, t in enumerate(sw.run_world(n, ag, flats)):
        for p in range(n):
            assert torch.equal(t.view(n, -1)[p], flats[p].view(n, -1)[p])


def test_mailbox_is_fifo_per_pair():
    """At n = 2 both ring neighbours are the same rank: two messages of
    one (sender, receiver) pair arrive in the order sent."""
    flats = [torch.full((4,), float(r)) for r in range(2)]

    def fn(comm, group, flat):
        other = 1 - comm.rank_in_comm
        a, b = torch.empty_like(flat), torch.empty_like(flat)
        comm.group_start()
        comm.send(flat, other)
        comm.send(flat + 10, other)
        comm.recv(a, other)
        comm.recv(b, other)
        comm.group_end()
        return a, b

    for r, (a, b) in enumerate(sw.run_world(2, fn, flats)):
        assert torch.equal(a, flats[1 - r])
        assert torch.equal(b, flats[1 - r] + 10)


def test_first_exception_is_reraised_without_hanging():
    flats = [torch.zeros(4) for _ in range(4)]

    def fn(comm, group, flat):
        if comm.rank_in_comm == 2:
            raise ValueError("rank 2 broke")
        comm.allgather_inplace(flat)

    with pytest.raises(ValueError, match="rank 2 broke"):
        sw.run_world(4, fn, flats)


# ---------------------------------------------------------------------------
# planted faults: the cases must be able to fail
# ---------------------------------------------------------------------------

_FAULT_GRID = [(3, torch.float32, 33), (8, torch.bfloat16, 4099)]


def _plant_wrong_target(monkeypatch, ops):
    reduce_, dqr = ops.reduce_chunk_inplace, ops.dequant_reduce
    monkeypatch.setattr(
        ops, "reduce_chunk_inplace",
        lambda flat, n, t, avg: reduce_(flat, n, (t + 1) % n, avg))
    monkeypatch.setattr(
        ops, "dequant_reduce",
        lambda buf, flat, n, t, avg: dqr(buf, flat, n, (t + 1) % n, avg))


def _plant_average_ignored(monkeypatch, ops):
    reduce_, dqr = ops.reduce_chunk_inplace, ops.dequant_reduce
    monkeypatch.setattr(
        ops, "reduce_chunk_inplace",
        lambda flat, n, t, avg: reduce_(flat, n, t, False))
    monkeypatch.setattr(
        ops, "dequant_reduce",
        lambda buf, flat, n, t, avg: dqr(buf, flat, n, t, False))


def _plant_second_compress_noop(monkeypatch, ops):
    compress = ops.compress_chunked

    def fake(flat, num_chunks, target_chunk=-1, out=None):
        if target_chunk >= 0:
            return out
        return compress(flat, num_chunks, target_chunk, out)

    monkeypatch.setattr(ops, "compress_chunked", fake)


@pytest.mark.parametrize("n,dtype,chunk", _FAULT_GRID,
                         ids=lambda v: sw._name(v)
                         if isinstance(v, torch.dtype) else str(v))
def test_planted_faults_are_caught(monkeypatch, n, dtype, chunk):
    from bagua_amd import executor

    with monkeypatch.context() as m:
        _plant_wrong_target(m, executor.ops)
        for case, args in [(sw.case_scattergather_exact, (True,)),
                           (sw.case_scattergather_random, (True,)),
                           (sw.case_bytegrad_exact, ()),
                           (sw.case_bytegrad_random, (True,))]:
            with pytest.raises(AssertionError):
                case(DEVICE, n, dtype, chunk, *args)

    with monkeypatch.context() as m:
        _plant_average_ignored(m, executor.ops)
        for case, args in [(sw.case_scattergather_exact, (True,)),
                           (sw.case_scattergather_random, (True,)),
                           (sw.case_bytegrad_exact, ()),
                           (sw.case_bytegrad_random, (True,))]:
            with pytest.raises(AssertionError):
                case(DEVICE, n, dtype, chunk, *args)

    with monkeypatch.context() as m:
        _plant_second_compress_noop(m, executor.ops)
        for case, args in [(sw.case_bytegrad_exact, ()),
                           (sw.case_bytegrad_random, (True,))]:
            with pytest.raises(AssertionError):
                case(DEVICE, n, dtype, chunk, *args)

    # with the faults lifted the same cases pass again
    sw.case_scattergather_exact(DEVICE, n, dtype, chunk, True)
    sw.case_bytegrad_exact(DEVICE, n, dtype, chunk)
