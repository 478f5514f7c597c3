"""The bucket sync protocols of bagua_amd/executor.py at world sizes 2, 3
and 8 on one GPU: N threads, one per simulated rank, drive the HIP
kernels through the unmodified protocol functions
(tests/internal/sim_world.py), with rank > 0 target chunks off 16-byte
alignment, a real chunk permutation between compress and dequant-reduce,
averaging by 1/3 and 1/8, requantization of a reduced chunk and carried
ring state. The cases, inputs and float64 bounds are those of
tests/test_sim_world.py, which passes them on the CPU with the torch
paths. GPU-only."""

import pytest
import torch

from tests.internal import sim_world as sw

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

DEVICE = "cuda"

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


@requires_gpu
def test_native_extension_is_what_runs():
    """The cuda world refuses to start without bagua_amd._C, and
    ``ops`` dispatches cuda tensors to it."""
    from bagua_amd import ops
    from bagua_amd.ops import native

    assert native.require() is not None
    assert ops._use_native(torch.zeros(4, device=DEVICE))


@requires_gpu
@grid
@averages
def test_scattergather_exact(n, dtype, chunk, average):
    sw.case_scattergather_exact(DEVICE, n, dtype, chunk, average)


@requires_gpu
@grid
@averages
def test_scattergather_random(n, dtype, chunk, average):
    sw.case_scattergather_random(DEVICE, n, dtype, chunk, average)


@requires_gpu
@grid
def test_bytegrad_exact(n, dtype, chunk):
    sw.case_bytegrad_exact(DEVICE, n, dtype, chunk)


@requires_gpu
@grid
@averages
def test_bytegrad_random(n, dtype, chunk, average):
    sw.case_bytegrad_random(DEVICE, n, dtype, chunk, average)


@requires_gpu
@even_grid
@pytest.mark.parametrize("exact", [False, True], ids=["random", "exact"])
def test_shift_one(n, dtype, chunk, exact):
    sw.case_shift_one(DEVICE, n, dtype, chunk, exact)


@requires_gpu
@grid
def test_low_prec_ring(n, dtype, chunk):
    sw.case_low_prec_ring(DEVICE, n, dtype, chunk)
